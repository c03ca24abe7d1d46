"""NumPy restatements of the policy target and of the legal-move cross-entropy (TEST INFRASTRUCTURE ONLY: not a test
module).  tests/test_policy_targets_cpu.py holds them against distributed.record_to_sample and a literal restatement of
_logits_to_move_probs (neural_network.py:148-169); tests/test_gpu_policy_targets.py uses them as the reference of
ReplayBuffer.sample_policy_tensors and training.policy_loss."""
import numpy as np

from chinesechessai_amd import _lib
from chinesechessai_amd.distributed import RECORD_DTYPE, unpack_board
from chinesechessai_amd.replay import pack_board_words

SLOTS = _lib.MAX_MOVES
N_MOVES = (1, 2, 63, 64, 65, 127, 128)                 # both sides of the 64-lane boundary and of the 128-slot cap


# ---- mirroring (file c -> 8 - c) -----------------------------------------------------------------------------------------
def mirror_square(s):
    s = np.asarray(s)
    return s - s % 9 + 8 - s % 9


def mirror_move(m):
    m = np.asarray(m, dtype=np.int64)
    return mirror_square(m // 90) * 90 + mirror_square(m % 90)


def mirror_board(board):
    return np.asarray(board).reshape(10, 9)[:, ::-1].copy()


def mirror_record(rec):
    """the record of the left-right mirrored sample: board and the first n_moves moves flipped, everything else kept"""
    out = np.array(rec, dtype=RECORD_DTYPE)
    out["board"] = pack_board_words(mirror_board(unpack_board(rec["board"])))
    n = int(rec["n_moves"])
    mv = out["moves"].copy()
    mv[:n] = mirror_move(rec["moves"][:n]).astype(np.uint16)
    out["moves"] = mv
    return out


# ---- the target: self_play.py:224-231, 234-239 ------------------------------------------------------------------------------
def target_pi64(counts, temperature):
    """float64 pi over the n moves of a record from its visit counts"""
    counts = np.asarray(counts).astype(np.int64)
    if temperature < 0.01:
        pi = np.zeros(len(counts))
        pi[np.argmax(counts)] = 1
        return pi
    c = counts ** (1.0 / temperature)
    return c / c.sum()


def target_of_record(rec, temperature, column_map=None, mirror=False):
    """(cols int32[128], pi float64[128], n): slots from n on are -1 / 0"""
    n = int(rec["n_moves"])
    mv = rec["moves"][:n].astype(np.int64)
    if mirror:
        mv = mirror_move(mv)
    cols = np.full(SLOTS, -1, np.int32)
    cols[:n] = mv if column_map is None else np.asarray(column_map)[mv]
    pi = np.zeros(SLOTS)
    if n:
        pi[:n] = target_pi64(rec["counts"][:n], temperature)
    return cols, pi, n


def make_record(board, moves, counts, z, player=1):
    r = np.zeros((), dtype=RECORD_DTYPE)
    n = len(moves)
    r["board"] = pack_board_words(board)
    r["z"] = z
    r["player"] = player
    r["n_moves"] = n
    r["valid"] = 1
    mv, ct = np.zeros(SLOTS, np.uint16), np.zeros(SLOTS, np.uint16)
    mv[:n], ct[:n] = moves, counts
    r["moves"], r["counts"] = mv, ct
    return r


# ---- the loss: neural_network.py:148-169 + cross-entropy ------------------------------------------------------------------
def literal_move_probs(logits, idx):
    """neural_network.py:148-169, literally, for the policy indices idx of the legal moves"""
    probs = np.array([logits[i] for i in idx])
    probs = np.exp(probs - np.max(probs))
    probs = probs / np.sum(probs)
    return probs


def loss_of_row(logits_row, cols, pi, n, dtype=np.float64):
    """(loss, resid[128], dense gradient[n_cols]) of one row in `dtype` arithmetic: the softmax over the usable slots
    (column >= 0), loss = -sum pi_i (x_i - max - log sum) over the slots with pi_i != 0, resid = p - pi"""
    n_cols = len(logits_row)
    resid = np.zeros(SLOTS, dtype)
    grad = np.zeros(n_cols, dtype)
    use = np.flatnonzero(np.asarray(cols[:n]) >= 0)
    if len(use) == 0:
        return dtype(0), resid, grad
    c = np.asarray(cols)[use].astype(np.int64)
    x = np.asarray(logits_row)[c].astype(dtype)
    t = np.asarray(pi)[use].astype(dtype)
    d = x - x.max()
    e = np.exp(d)
    s = e.sum(dtype=dtype)
    lg = np.log(s)
    nz = t != 0
    loss = -(t[nz] * (d[nz] - lg)).sum(dtype=dtype)
    resid[use] = e / s - t
    np.add.at(grad, c, resid[use])
    return dtype(loss), resid, grad
