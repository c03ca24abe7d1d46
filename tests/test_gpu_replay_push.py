"""GPU tests (`-m gpu`, through the C ABI) of xq_replay_push_records past 1,024 games - where every thread of k_scan's one
workgroup carries more than one game - and with valid flags that are not a prefix of a game's plies.  Reference:
tests/row_model.DequeRing = collections.deque(maxlen) (checked against brute-force loops by tests/test_row_model_cpu.py).

Records are hand-made (no engine): the value target z of a record is its tag (first_game + game) * 128 + ply, an integer
below 2^24 and so exact in the float32 target of sample_tensors; its board holds one piece (code 5) on square tag % 90.  The
ring is read back both ways: xq_replay_read_records (the raw records) and sample_tensors(indices=arange(len)) (the batch
formation the trainer uses)."""
import ctypes as C

import numpy as np
import pytest

from tests import row_model as rm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


def _records(valid, first_game):
    """xq_sample_record[n_games][70] on the device for valid[n_games][70]; the records that are NOT valid carry a tag of
    their own too (z = -tag - 1, a board): pushing one of them shows"""
    import torch
    from chinesechessai_amd.distributed import RECORD_DTYPE
    n = len(valid)
    rec = np.zeros((n, rm.MAX_PLIES), dtype=RECORD_DTYPE)
    tag = (np.arange(n)[:, None] + first_game) * 128 + np.arange(rm.MAX_PLIES)[None, :]
    sq = tag % 90
    rec["z"] = np.where(valid, tag, -tag - 1).astype(np.float64)
    rec["valid"] = valid
    rec["player"] = np.where(tag % 2 == 0, 1, -1)
    rec["n_moves"] = 1
    rec["moves"][..., 0] = tag % 8100
    rec["counts"][..., 0] = 1 + tag % 7
    words = np.zeros((n, rm.MAX_PLIES, 12), np.uint32)
    np.put_along_axis(words, (sq // 8)[..., None], (np.uint32(5) << (4 * (sq % 8)).astype(np.uint32))[..., None], axis=2)   # piece code 5
    rec["board"] = words
    return torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).cuda(), rec


def _read_all(buf):
    from chinesechessai_amd import _lib
    from chinesechessai_amd.distributed import RECORD_DTYPE
    n = len(buf)
    idx = np.arange(n, dtype=np.int64)
    out = np.zeros(max(n, 1), dtype=RECORD_DTYPE)
    if n:
        buf._chk(buf.L.xq_replay_read_records(buf.h, C.c_void_p(buf._stream()), _lib.ptr(idx), n, _lib.ptr(out)))
    return out[:n]


def _check_ring(buf, ring, sources, tag):
    """the device ring against the model: length, order, every record byte for byte, and the trainer's view of it"""
    import torch
    want = ring.tags()
    assert len(buf) == len(ring) == len(want), "%s: len %d, want %d" % (tag, len(buf), len(want))
    got = _read_all(buf)
    got_tags = got["z"].astype(np.int64)
    bad = np.nonzero(got_tags != want)[0]
    assert len(bad) == 0, "%s: %d of %d ring entries differ, first at deque index %d: tag %d, want %d" % (
        tag, len(bad), len(want), bad[0], got_tags[bad[0]], want[bad[0]])
    # every record byte for byte: the source record of each tag
    for first, rec in sources:
        g = want // 128 - first
        sel = (g >= 0) & (g < len(rec))
        if sel.any():
            src = rec[g[sel], want[sel] % 128]
            assert got[sel].tobytes() == src.tobytes(), "%s: record bytes differ" % (tag,)
    covered = np.zeros(len(want), bool)
    for first, rec in sources:
        g = want // 128 - first
        covered |= (g >= 0) & (g < len(rec))
    assert covered.all()
    if len(want):
        states, targets = buf.sample_tensors(len(want), indices=np.arange(len(want)))
        t = torch.from_numpy(want).cuda()
        assert torch.equal(targets.reshape(-1), t.to(torch.float32)), tag
        king = states[:, 4].reshape(len(want), 90)                   # plane 4: piece code 5
        assert torch.equal(king.argmax(dim=1), t % 90) and bool((states[:, :14].sum(dim=(1, 2, 3)) == 1).all()), tag


def _pushes(valid, flags):
    """a push of 3 games (so that the tail is not 0), the push under test, one more push of 5 games of the same family
    (so that a small ring wraps twice): [(valid, first_game, device records, host records)], built once per test"""
    out, first = [], 0
    for v in (rm.prefix_flags(3, seed=1), valid, flags(5, seed=2)):
        dev, rec = _records(v, first)
        out.append((v, first, dev, rec))
        first += len(v)
    return out


def _session(pushes, cap, tag):
    """the three pushes into a ring of `cap` records; the ring is compared with the model after each"""
    from chinesechessai_amd.replay import ReplayBuffer
    buf, ring, sources = ReplayBuffer(max_size=cap), rm.DequeRing(cap), []
    try:
        for i, (v, first, dev, rec) in enumerate(pushes):
            sources.append((first, rec))
            n = buf.push_records(dev, len(v))
            want = ring.push(v, first_game=first)
            assert n == len(want) == int(v.sum()), "%s push %d: n_pushed %d, want %d" % (tag, i, n, len(want))
            _check_ring(buf, ring, sources, "%s after push %d" % (tag, i))
    finally:
        buf.close()


def _caps(total):
    return (1, 7, 70, total - 1, total, total + 1, 5 * total)


@pytest.mark.parametrize("n_games", (1024, 1025, 2047, 2049, 3073))
def test_push_past_one_game_per_scan_thread(L, n_games):
    """Ragged prefix lengths 0 .. 70 (six games in ten empty) over 1,024 .. 3,073 games: k_scan's threads carry 1, 2, 2, 3
    and 4 games each, the last thread a short share.  Capacities 1, 7, 70, total - 1, total, total + 1 and 5 x total; every push
    is preceded by one of 3 games and followed by one of 5.  n_pushed, len, the order and every record equal the deque.
    Every valid flag here is part of a prefix: the library from before k_push learnt to skip gaps passes this test too, so
    prefix input - all the engine writes - lands in the same ring bytes as before."""
    valid = rm.prefix_flags(n_games)
    total = int(valid.sum())
    pushes = _pushes(valid, rm.prefix_flags)
    for cap in _caps(total):
        _session(pushes, cap, "n_games %d cap %d" % (n_games, cap))


@pytest.mark.parametrize("n_games", (5, 1025))
def test_push_skips_gaps_and_drops_nothing_behind_them(L, n_games):
    """Games whose valid flags are not a prefix - first ply invalid, every second ply, one hole in the middle, only ply 69 -
    mixed with prefix games: "push every valid record ... in game / ply order".  k_count_valid counts every valid record;
    k_push used to stop at a game's first invalid ply and to place records by ply index, so that the ring's length and
    head ran over slots nobody wrote and the records behind a gap were lost."""
    valid = rm.gap_flags(n_games)
    total = int(valid.sum())
    pushes = _pushes(valid, rm.gap_flags)
    for cap in _caps(total):
        _session(pushes, cap, "gaps, n_games %d cap %d" % (n_games, cap))


def test_a_push_of_empty_games_changes_nothing(L):
    from chinesechessai_amd.replay import ReplayBuffer
    buf, ring = ReplayBuffer(max_size=50), rm.DequeRing(50)
    try:
        v = rm.prefix_flags(3, seed=1)
        dev, rec = _records(v, 0)
        assert buf.push_records(dev, 3) == len(ring.push(v))
        before = _read_all(buf).tobytes()
        empty = np.zeros((1030, rm.MAX_PLIES), bool)
        dev2, rec2 = _records(empty, 3)
        assert buf.push_records(dev2, len(empty)) == 0 == len(ring.push(empty, first_game=3))
        assert _read_all(buf).tobytes() == before
        _check_ring(buf, ring, [(0, rec)], "after an empty push")
    finally:
        buf.close()
