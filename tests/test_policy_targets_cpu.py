"""Policy targets and the legal-move loss, the parts that need no GPU: the boundary (header, library, ctypes table), the
loud failure without a device, and the NumPy restatements of tests/policy_reference.py - the reference of the GPU tests -
held against the package's own host code and a literal restatement of the reference's softmax."""
import os
import re

import numpy as np
import pytest

from chinesechessai_amd import _lib
from chinesechessai_amd.chess_env import decode_move
from chinesechessai_amd.distributed import record_to_sample, unpack_board
from tests import policy_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("xq_replay_encode_policy_batch", "xq_policy_loss_f32", "xq_policy_loss_grad_f32")
TEMPERATURES = (1.0, 0.5, 0.7, 0.001)


def _records(rng):
    """one record per n_moves of pr.N_MOVES and per kind of counts: ordinary with zeros among them, a single non-zero,
    a tie for the maximum, and the largest count a record holds"""
    out = []
    for n in pr.N_MOVES:
        moves = rng.choice(8100, n, replace=False)
        board = rng.randint(-7, 8, size=(10, 9)).astype(np.int8)
        kinds = {"zeros": np.where(rng.random_sample(n) < 0.4, 0, rng.randint(1, 50, n)),
                 "single": np.zeros(n, np.int64),
                 "tie": rng.randint(0, 20, n),
                 "big": rng.randint(0, 65536, n)}
        kinds["zeros"][n - 1] = 3
        kinds["single"][n // 2] = 17
        kinds["tie"][[n // 3, n - 1]] = 40
        kinds["big"][0] = 65535
        for kind, counts in kinds.items():
            out.append((n, kind, pr.make_record(board, moves, counts, 0.5)))
    return out


def test_new_entry_points_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "xq_selfplay.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr) and hasattr(L, name), name
    assert any(s.endswith("xq_policy_loss.hip") for s in _lib.SOURCES)
    # the header comment cites what the entry point replaces
    doc = hdr[:hdr.index("int     xq_replay_encode_policy_batch")]
    doc = doc[doc.rindex("/*"):]
    for cite in ("trainer.py:313-331", "self_play.py:234-239", "neural_network.py:160"):
        assert cite in doc, cite


def test_without_a_gpu_nothing_falls_back():
    import torch
    from chinesechessai_amd import training
    from chinesechessai_amd.replay import PolicyTarget, ReplayBuffer
    assert callable(ReplayBuffer.sample_policy_tensors)
    target = PolicyTarget(torch.full((2, 128), -1, dtype=torch.int32), torch.zeros(2, 128), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="CUDA"):                 # host tensors: no kernel covers them, nothing else runs
        training.policy_loss(torch.zeros(2, 8100), target)
    with pytest.raises(ValueError):
        training.policy_loss(torch.zeros(2, 8100), target, reduction="median")
    if _lib.lib().xq_device_count() == 0:
        with pytest.raises(_lib.XqError):                         # no device, no buffer, hence no sample_policy_tensors
            ReplayBuffer(max_size=8)
        assert _lib.lib().xq_replay_encode_policy_batch(None, None, None, 1, None, 0, 1.0, None, 0, None, None, None,
                                                        None, None, None) == -1
        assert _lib.lib().xq_policy_loss_f32(None, None, 8100, 8100, None, None, None, 1, None, None) == -1
        assert _lib.lib().xq_policy_loss_grad_f32(None, None, None, None, None, 1.0, 1, None, 8100, 8100) == -1


@pytest.mark.parametrize("temperature", TEMPERATURES)
def test_target_restatement_equals_record_to_sample(temperature):
    rng = np.random.RandomState(11)
    for n, kind, rec in _records(rng):
        cols, pi, n_out = pr.target_of_record(rec, temperature)
        board, probs, z = record_to_sample(rec, temperature)
        assert n_out == n == len(probs) and z == 0.5 and np.array_equal(board, unpack_board(rec["board"]))
        assert [decode_move(int(c)) for c in cols[:n]] == list(probs.keys()), (n, kind)
        assert pi[:n].tobytes() == np.array(list(probs.values()), np.float64).tobytes(), (n, kind)
        assert (cols[n:] == -1).all() and (pi[n:] == 0).all()
        if temperature < 0.01:
            first = int(np.flatnonzero(rec["counts"][:n] == rec["counts"][:n].max())[0])
            assert pi[first] == 1 and pi.sum() == 1, (n, kind)


def test_exact_temperatures_sum_integers():
    """at T = 1 and T = 0.5 every power and every partial sum is an integer below 2**53: any order of summation gives
    the same float64, which is why the GPU test may ask for equal bits there"""
    rng = np.random.RandomState(12)
    for n, kind, rec in _records(rng):
        c = rec["counts"][:n].astype(np.int64)
        for T, exact in ((1.0, c), (0.5, c * c)):
            p = c ** (1.0 / T)
            assert np.array_equal(p, exact.astype(np.float64)) and int(exact.sum()) < 2 ** 53
            assert p.sum() == float(int(exact.sum())) == p[::-1].sum()


def test_column_map_and_mirror_in_the_target():
    from chinesechessai_amd.neural_network import reachable_policy_columns
    _, cmap = reachable_policy_columns()
    rng = np.random.RandomState(13)
    for n, kind, rec in _records(rng):
        plain = pr.target_of_record(rec, 1.0)
        mapped = pr.target_of_record(rec, 1.0, column_map=cmap)
        assert np.array_equal(mapped[0][:n], cmap[rec["moves"][:n].astype(np.int64)]) and (mapped[0][n:] == -1).all()
        assert mapped[1].tobytes() == plain[1].tobytes()
        flipped = pr.target_of_record(rec, 1.0, mirror=True)
        assert flipped[1].tobytes() == plain[1].tobytes()             # pi does not move
        assert np.array_equal(flipped[0], pr.target_of_record(pr.mirror_record(rec), 1.0)[0])
        twice = pr.mirror_record(pr.mirror_record(rec))
        assert twice.tobytes() == rec.tobytes()


def test_loss_restatement_equals_the_reference_softmax():
    """float64: p of loss_of_row (through resid + pi) is _logits_to_move_probs of the same logits, bit for bit when no
    column is masked out; the loss is -sum pi log p; the dense gradient is resid scattered to the columns"""
    rng = np.random.RandomState(14)
    for n_cols in (8100, 2304):
        for n in pr.N_MOVES:
            logits = rng.standard_normal(n_cols) * (80.0 if n == 65 else 1.0)
            cols = np.full(128, -1, np.int32)
            cols[:n] = rng.choice(n_cols, n, replace=False)
            pi = np.zeros(128)
            pi[:n] = rng.random_sample(n) * (rng.random_sample(n) < 0.7)
            pi[n - 1] += 0.1
            pi /= pi.sum()
            loss, resid, grad = pr.loss_of_row(logits, cols, pi, n)
            p = pr.literal_move_probs(logits, cols[:n])
            assert (resid[:n] + pi[:n] - p).tobytes() == np.zeros(n).tobytes() or np.abs(resid[:n] + pi[:n] - p).max() < 2e-16
            nz = pi[:n] != 0
            assert abs(loss + (pi[:n][nz] * np.log(p[nz])).sum()) <= 1e-12 * max(1.0, abs(loss))
            assert np.array_equal(grad[cols[:n]], resid[:n]) and np.count_nonzero(grad) <= n
            assert (resid[n:] == 0).all()
    # a masked column takes part in nothing; a row without a usable slot is all zero
    logits = rng.standard_normal(50)
    cols = np.full(128, -1, np.int32)
    cols[:4] = [3, -1, 7, 49]
    pi = np.zeros(128)
    pi[:4] = [0.25, 0.5, 0.25, 0.0]
    loss, resid, grad = pr.loss_of_row(logits, cols, pi, 4)
    p = pr.literal_move_probs(logits, [3, 7, 49])
    assert np.allclose(resid[[0, 2, 3]], p - [0.25, 0.25, 0.0], atol=1e-15) and resid[1] == 0
    assert np.isclose(loss, -0.25 * np.log(p[0]) - 0.25 * np.log(p[1]))
    loss, resid, grad = pr.loss_of_row(logits, cols, pi, 0)
    assert loss == 0 and not resid.any() and not grad.any()


def test_mirroring_is_an_involution_and_keeps_moves_reachable(golden_dir):
    from chinesechessai_amd.neural_network import reachable_policy_columns
    from oracle import xq_oracle as xo
    _, cmap = reachable_policy_columns()
    allm = np.arange(8100)
    assert np.array_equal(pr.mirror_move(pr.mirror_move(allm)), allm)
    assert np.array_equal(np.sort(pr.mirror_move(allm)), allm)            # a permutation of the policy indices
    assert np.array_equal(cmap[pr.mirror_move(allm)] >= 0, cmap >= 0)     # ... that maps the reachable set onto itself
    d = np.load(os.path.join(golden_dir, "rules_random.npz"))
    for i in range(len(d["nlegal"])):
        mv = d["legal"][i, :d["nlegal"][i]].astype(np.int64)
        assert (cmap[pr.mirror_move(mv)] >= 0).all(), i
        b = d["board"][i].reshape(10, 9)
        assert np.array_equal(pr.mirror_board(pr.mirror_board(b)), b)
    # the rules are symmetric under the flip: the mirrored position's legal moves are the mirrored legal moves
    for i in range(0, len(d["nlegal"]), 97):
        oe = xo.OracleEnv()
        rk, bk = int(d["red_king"][i]), int(d["black_king"][i])
        oe.set_state(pr.mirror_board(d["board"][i]).reshape(90), int(d["player"][i]),
                     red_king=int(pr.mirror_square(rk)) if rk >= 0 else rk,
                     black_king=int(pr.mirror_square(bk)) if bk >= 0 else bk)
        want = sorted(pr.mirror_move(d["legal"][i, :d["nlegal"][i]]).tolist())
        assert sorted(oe.legal_moves()) == want, i
