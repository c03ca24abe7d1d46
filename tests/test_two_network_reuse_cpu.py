"""CPU suite for the evaluation cache and the root carry-over in two-network sessions (xq_engine_set_per_slot_reuse,
SelfPlayEngine.set_per_slot_reuse, play_refill(reuse=) / self_play_epoch(reuse=)): the entry point is declared and bound,
and every argument error is raised before any device call."""
import os
import re

import numpy as np
import pytest

from chinesechessai_amd import _lib
from chinesechessai_amd.engine import (CallbackEvaluator, HashNetEvaluator, SelfPlayEngine, check_keep_plies,
                                       check_reuse_evaluators)
from chinesechessai_amd.self_play import self_play_epoch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Net:
    """a reference-style network object: the mirror wraps it into a CallbackEvaluator"""

    def predict_batch(self, rows):
        raise AssertionError("no evaluation may happen in these tests")


class _NoDevice:
    """stands in for the loaded library: any call into it fails the test"""

    def __getattr__(self, name):
        raise AssertionError("%s was called before the arguments were checked" % name)


def _engine_without_a_device():
    eng = SelfPlayEngine.__new__(SelfPlayEngine)
    eng.L, eng.h = _NoDevice(), None
    eng.n_games, eng.opponent_mode = 4, False
    eng.root_eval_carry, eng._carry_on, eng._slot_reuse = None, False, False
    return eng


def test_the_entry_point_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "xq_selfplay.h")).read()
    assert re.search(r"\bint\s+xq_engine_set_per_slot_reuse\s*\(\s*xq_engine\s*\*\s*e\s*,\s*int\s+enable\s*,\s*int\s+keep_plies\s*\)\s*;", hdr)
    assert "xq_engine_set_per_slot_reuse" in _lib.EXPORTS
    res, args = _lib._SIGNATURES["xq_engine_set_per_slot_reuse"]
    assert len(args) == 3
    # its comment names the reference lines it answers to, like its neighbours'
    doc = hdr[:hdr.index("xq_engine_set_per_slot_reuse(xq_engine")].rsplit("/*", 1)[1]
    assert "self_play.py:98" in doc and "trainer.py:186-209" in doc and "keep_plies" in doc


@pytest.mark.parametrize("bad", [0, 1, 4, -3, 2.5, None, True])
def test_keep_plies_outside_2_and_3_raises_before_any_device_call(bad):
    eng = _engine_without_a_device()
    with pytest.raises(ValueError, match="keep_plies"):
        eng.set_per_slot_reuse(True, keep_plies=bad)
    with pytest.raises(ValueError, match="keep_plies"):
        eng.set_per_slot_reuse(False, keep_plies=bad)
    assert not eng._slot_reuse
    assert check_keep_plies(2) == 2 and check_keep_plies(3) == 3


def test_reuse_with_a_callback_evaluator_raises_before_any_device_call(monkeypatch):
    check_reuse_evaluators(HashNetEvaluator(0), HashNetEvaluator(1))
    for pair in ((CallbackEvaluator(_Net()), HashNetEvaluator(1)), (HashNetEvaluator(0), CallbackEvaluator(_Net()))):
        with pytest.raises(_lib.XqError, match="reuse=True"):
            check_reuse_evaluators(*pair)
        eng = _engine_without_a_device()
        with pytest.raises(_lib.XqError, match="reuse=True"):
            eng.play_refill(pair[0], np.arange(4, dtype=np.uint32), 0, opponent_evaluator=pair[1], reuse=True)
    from chinesechessai_amd import self_play as sp

    def no_engine(*a, **k):
        raise AssertionError("the engine was created before the arguments were checked")
    monkeypatch.setattr(sp, "SelfPlayEngine", no_engine)
    with pytest.raises(_lib.XqError, match="reuse=True"):
        self_play_epoch(_Net(), 4, 1.0, 16, opponent_network=_Net(), reuse=True)
    with pytest.raises(_lib.XqError, match="reuse=True"):
        self_play_epoch(HashNetEvaluator(0), 4, 1.0, 16, opponent_network=_Net(), reuse=True)
    # without reuse the message is the per-slot session's own, as before
    with pytest.raises(_lib.XqError, match="per-slot two-network session"):
        self_play_epoch(HashNetEvaluator(0), 4, 1.0, 16, opponent_network=_Net())


def test_self_play_epoch_reuse_without_an_opponent_is_plain_self_play(monkeypatch):
    """reuse=True without an opponent: the same argument handling as without it, and the session is not asked to reuse"""
    from chinesechessai_amd import self_play as sp
    asked = []

    class _Engine:
        def __init__(self, slots, **kw):
            asked.append(("engine", slots))

        def play_refill(self, ev, seeds, ptr, opponent_evaluator=None, pairing=None, reuse=False):
            asked.append(("play_refill", opponent_evaluator, pairing, reuse))
            raise AssertionError("as far as the session and no further")

        def close(self):
            pass

    def no_engine(*a, **k):
        raise AssertionError("the engine was created before the arguments were checked")
    monkeypatch.setattr(sp, "SelfPlayEngine", no_engine)
    with pytest.raises(ValueError, match="num_games"):
        self_play_epoch(HashNetEvaluator(0), 0, 1.0, 16, reuse=True)
    with pytest.raises(ValueError, match="seeds"):
        self_play_epoch(HashNetEvaluator(0), 4, 1.0, 16, seeds=[1, 2, 3], reuse=True)
    # a reference-style network alone is plain self-play: reuse does not refuse it
    with pytest.raises(AssertionError, match="engine was created"):
        self_play_epoch(_Net(), 4, 1.0, 16, reuse=True)
    with pytest.raises(AssertionError, match="engine was created"):
        self_play_epoch(HashNetEvaluator(0), 4, 1.0, 16, slots=9, reuse=True)
    import torch
    monkeypatch.setattr(sp, "SelfPlayEngine", _Engine)
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: type("T", (), {"data_ptr": lambda self: 0})())
    with pytest.raises(AssertionError, match="no further"):
        self_play_epoch(HashNetEvaluator(0), 4, 1.0, 16, slots=2, seeds=[1, 2, 3, 4], reuse=True)
    assert asked[0] == ("engine", 2)
    assert asked[1][1] is None and asked[1][2] is None and asked[1][3] is False
    # ... and with an opponent it is passed on
    del asked[:]
    with pytest.raises(AssertionError, match="no further"):
        self_play_epoch(HashNetEvaluator(0), 4, 1.0, 16, opponent_network=HashNetEvaluator(1), slots=2, seeds=[1, 2, 3, 4],
                        reuse=True)
    assert asked[1][3] is True and asked[1][2].tolist() == [0, 0, 1, 1]
