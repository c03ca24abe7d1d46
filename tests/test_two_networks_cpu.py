"""CPU suite for the two-network surface: self_play_epoch's argument handling, the num_games // 2 split and the errors
a per-slot session raises before any device call (the device is first touched when the engine is created)."""
import numpy as np
import pytest

from chinesechessai_amd import _lib
from chinesechessai_amd.engine import (CallbackEvaluator, HashNetEvaluator, check_per_slot_evaluators,
                                       normalise_pairing)
from chinesechessai_amd.self_play import epoch_pairing, self_play_epoch


class _Net:
    """a reference-style network object: the mirror wraps it into a CallbackEvaluator"""

    def predict_batch(self, rows):
        raise AssertionError("no evaluation may happen in these tests")


def test_epoch_split_is_the_trainers():
    """trainer.py:156-163: num_games // 2 self-play games first, the rest against the old model"""
    assert epoch_pairing(6, True).tolist() == [0, 0, 0, 1, 1, 1]
    assert epoch_pairing(7, True).tolist() == [0, 0, 0, 1, 1, 1, 1]
    assert epoch_pairing(1, True).tolist() == [1]
    assert epoch_pairing(5, False).tolist() == [0] * 5
    assert epoch_pairing(6, True).dtype == np.uint8


def test_pairing_is_checked_on_the_host():
    assert normalise_pairing(None, 4, False) is None
    assert normalise_pairing(None, 4, True).tolist() == [1, 1, 1, 1]
    p = normalise_pairing([0, 1, 0, 1], 4, True)
    assert p.dtype == np.uint8 and p.tolist() == [0, 1, 0, 1]
    assert normalise_pairing([0, 0], 2, False).tolist() == [0, 0]
    with pytest.raises(ValueError, match="one entry per game"):
        normalise_pairing([0, 1, 0], 4, True)
    with pytest.raises(ValueError, match="0 .self-play. or 1"):
        normalise_pairing([0, 2, 0, 1], 4, True)
    with pytest.raises(ValueError, match="needs an opponent"):
        normalise_pairing([0, 1, 0, 1], 4, False)


def test_callback_evaluators_are_refused_in_a_per_slot_session():
    check_per_slot_evaluators(HashNetEvaluator(0), HashNetEvaluator(1))
    for pair in ((CallbackEvaluator(_Net()), HashNetEvaluator(1)), (HashNetEvaluator(0), CallbackEvaluator(_Net()))):
        with pytest.raises(_lib.XqError, match="CallbackEvaluator"):
            check_per_slot_evaluators(*pair)


def test_self_play_epoch_errors_come_before_any_device_call(monkeypatch):
    """every argument error is raised while no engine exists: creating one is made to fail the test"""
    from chinesechessai_amd import self_play as sp

    def no_engine(*a, **k):
        raise AssertionError("the engine was created before the arguments were checked")
    monkeypatch.setattr(sp, "SelfPlayEngine", no_engine)
    with pytest.raises(ValueError, match="num_games"):
        self_play_epoch(HashNetEvaluator(0), 0, 1.0, 16)
    with pytest.raises(ValueError, match="slots"):
        self_play_epoch(HashNetEvaluator(0), 4, 1.0, 16, slots=0)
    with pytest.raises(ValueError, match="seeds"):
        self_play_epoch(HashNetEvaluator(0), 4, 1.0, 16, seeds=[1, 2, 3])
    with pytest.raises(_lib.XqError, match="CallbackEvaluator"):
        self_play_epoch(_Net(), 4, 1.0, 16, opponent_network=_Net())
    with pytest.raises(_lib.XqError, match="CallbackEvaluator"):
        self_play_epoch(HashNetEvaluator(0), 4, 1.0, 16, opponent_network=_Net())
    # valid arguments get as far as the engine (and no further here)
    with pytest.raises(AssertionError, match="engine was created"):
        self_play_epoch(HashNetEvaluator(0), 4, 1.0, 16, opponent_network=HashNetEvaluator(1), slots=9)
