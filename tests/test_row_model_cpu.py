"""CPU checks of tests/row_model.py: the host models the GPU tests compare k_assign_rows and xq_replay_push_records with
are themselves compared with brute-force loops, over the very masks and flag arrays the GPU tests use, and those masks
are shown to exercise what they are for (no pass or wave boundary carries zero by accident)."""
import collections

import numpy as np
import pytest

from tests import row_model as rm


def _number_rows_loops(pending, net1, dup_of, cached):
    n = len(pending)
    leaf_row = [-1] * n
    src = ([], [])
    for s in range(n):
        if not pending[s] or (cached is not None and cached[s]):
            continue
        k = 1 if (net1 is not None and net1[s]) else 0
        if dup_of is not None and dup_of[s] >= 0 and dup_of[s] != s:
            leaf_row[s] = leaf_row[int(dup_of[s])]              # the group's lowest slot: numbered before this one
        else:
            leaf_row[s] = len(src[k])
            src[k].append(s)
    return leaf_row, src[0], src[1]


def _same(model, loops):
    lr, s0, s1, c0, c1 = model
    assert lr.dtype == np.int32 and lr.tolist() == loops[0]
    assert s0.tolist() == loops[1] and s1.tolist() == loops[2] and (c0, c1) == (len(loops[1]), len(loops[2]))


@pytest.mark.parametrize("n", rm.SLOT_COUNTS)
def test_number_rows_equals_the_loops_on_every_mask_family(n):
    for kind in rm.MASK_KINDS:
        live = rm.make_mask(kind, n)
        assert live.shape == (n,) and live.dtype == bool          # (random03 may be empty at the smallest counts: 0 rows)
        _same(rm.number_rows(live), _number_rows_loops(live, None, None, None))
        rng = np.random.default_rng(n)
        net1 = rng.random(n) < 0.5
        _same(rm.number_rows(live, net1=net1), _number_rows_loops(live, net1, None, None))
        cached = rng.random(n) < 0.2
        _same(rm.number_rows(live, net1=net1, cached=cached), _number_rows_loops(live, net1, None, cached))
        # groups of equal positions inside each network
        pos = rng.integers(0, 12, n)
        dup = rm.dup_of_groups(live, [(int(p), bool(k)) for p, k in zip(pos, net1)])
        got = rm.number_rows(live, net1=net1, dup_of=dup)
        _same(got, _number_rows_loops(live, net1, dup, None))
        rows = got[0]
        assert ((rows >= 0) == live).all()
        for k, srck in ((False, got[1]), (True, got[2])):
            assert (np.diff(srck) > 0).all()                    # rows in the order of each group's lowest slot
            assert (rows[srck] == np.arange(len(srck))).all()
            if live.any() and n > 64:
                # same (position, network) <=> same row
                sel = np.nonzero(live & (net1 == k))[0]
                assert len(set(zip(pos[sel].tolist(), rows[sel].tolist()))) == len(set(pos[sel].tolist())) == len(set(rows[sel].tolist()))


@pytest.mark.parametrize("n", rm.SLOT_COUNTS)
def test_masks_mix_every_wave_span(n):
    """Within every 16,384-slot pass, every 1,024-slot wave span inside the slots holds a live and a dead slot - for the
    families that promise it; "all" and "boundaries" are the two extremes on purpose, and are what they say."""
    for kind in rm.MIXED_KINDS:
        assert rm.mixed_spans(rm.make_mask(kind, n)), (kind, n)
    assert rm.make_mask("all", n).all()
    b = rm.make_mask("boundaries", n)
    want = sorted({0, n - 1} | {x for p in rm.pass_boundaries(n) for x in (p - 1, p)})
    assert np.nonzero(b)[0].tolist() == want
    assert (n > rm.PASS) == (len(rm.pass_boundaries(n)) > 0)
    # the checker itself: a span of one kind fails it
    if n >= rm.SPAN:
        for fill in (False, True):
            m = rm.make_mask("random50", n)
            m[:rm.SPAN] = fill
            assert not rm.mixed_spans(m)


@pytest.mark.parametrize("n", (16401, 32785))
def test_dedupe_assignment_spans_the_passes(n):
    live, pos = rm.dedupe_assignment(n, 12)
    assert rm.mixed_spans(live)
    first = {}
    for s in np.nonzero(live)[0]:
        first.setdefault(int(pos[s]), int(s))
    assert sorted(first) == list(range(12)) and max(first.values()) < rm.PASS        # every group's lowest slot: pass 0
    for p0 in range(rm.PASS, n, rm.PASS):                                            # ... and members in every later pass
        sel = live[p0:p0 + rm.PASS]
        assert set(pos[p0:p0 + rm.PASS][sel].tolist()) == set(range(12))


@pytest.mark.parametrize("n", (17, 16401, 32785))
def test_two_network_masks_mix_both_networks(n):
    """the two-network cases: random50 slots, random networks - every whole wave span holds rows of both networks, so that
    neither half of the packed scan word carries zero over a boundary"""
    live = rm.make_mask("random50", n)
    net1 = rm.two_network_split(n)
    for s0 in range(0, n - rm.SPAN + 1, rm.SPAN):
        sl = slice(s0, s0 + rm.SPAN)
        assert (live[sl] & net1[sl]).any() and (live[sl] & ~net1[sl]).any()


def _deque_loops(cap, pushes):
    d = collections.deque(maxlen=cap)
    out = []
    for valid, first in pushes:
        tags = []
        for g in range(len(valid)):
            for p in range(rm.MAX_PLIES):
                if valid[g][p]:
                    tags.append((first + g) * 128 + p)
        d.extend(tags)
        out.append(tags)
    return list(d), out


@pytest.mark.parametrize("n_games", (5, 1024, 1025, 2047, 2049, 3073))
def test_deque_ring_equals_a_deque(n_games):
    for flags in (rm.prefix_flags, rm.gap_flags):
        valid = flags(n_games)
        total = int(valid.sum())
        assert total > 70
        pushes = [(rm.prefix_flags(3, seed=1), 0), (valid, 3), (flags(5, seed=2), 3 + n_games)]   # as tests/test_gpu_replay_push.py pushes
        for cap in (1, 7, 70, total - 1, total, total + 1, 5 * total):
            ring = rm.DequeRing(cap)
            got = [ring.push(v, first_game=f).tolist() for v, f in pushes]
            want, want_pushed = _deque_loops(cap, pushes)
            assert got == want_pushed and ring.tags().tolist() == want and len(ring) == len(want)
    # what the generators promise
    pre = rm.prefix_flags(n_games)
    assert (np.diff(pre.astype(int), axis=1) <= 0).all()                    # prefixes
    assert pre.sum(axis=1).max() == 70 and pre[-1].sum() == 1
    gap = rm.gap_flags(n_games)
    nonprefix = (np.diff(gap.astype(int), axis=1) > 0).any(axis=1) | (~gap[:, 0] & gap.any(axis=1))
    assert nonprefix.sum() >= min(4, n_games - 1)
    assert not gap[0, 0] and gap[3].sum() == 1 and gap[3, 69]                # first ply invalid; only ply 69
    assert (3 + n_games + 5) * 128 < 2 ** 24                                 # every tag is exact in float32
    if n_games >= 1024:
        assert (pre.sum(axis=1) == 0).mean() > 0.4                          # many empty games


def test_an_empty_push_changes_nothing():
    ring = rm.DequeRing(10)
    ring.push(rm.prefix_flags(3, seed=1))
    before = ring.tags().tolist()
    assert len(ring.push(np.zeros((4, 70), bool), first_game=9)) == 0 and ring.tags().tolist() == before
