"""CPU suite for the trunk kernel's permuted MFMA columns (tools/gen_tower1wa.py: PIX_OF, DEAD, SKIP): the tables are
re-derived here from the board's geometry alone, the generated stream leaves out exactly the MFMAs of the all-padding
(pixel tile, tap) pairs, and the symbolic checker notices one MFMA too few or too many."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RANKS, FILES = 10, 9


def _valid(p, tap):
    """pixel p = 9 rank + file has the neighbour (rank + tap // 3 - 1, file + tap % 3 - 1) on the 10 x 9 board"""
    if p < 0:
        return False
    y, x = p // FILES + tap // 3 - 1, p % FILES + tap % 3 - 1
    return 0 <= y < RANKS and 0 <= x < FILES


def _linear(g):
    n = 3
    pro = g.sec_pro(False)
    even = [g.sec_even(False, b) for b in range(n)]
    odd = [g.sec_odd(False, b) for b in range(n)]
    x2 = [g.sec_x2(False, b) for b in range(n)]
    fin = g.sec_fin(False, n - 1)
    lin = [g.Ins("", "blk", blk=0)] + list(pro.ins)
    for b in range(n):
        lin += [g.Ins("", "blk", blk=b)] + even[b].ins + odd[b].ins
        lin += x2[b].ins if b < n - 1 else fin.ins
    return g.insert_lgkm_waits(lin)


def test_columns_are_a_bijection_onto_the_board_plus_six_pads():
    import gen_tower1wa as g
    assert len(g.PIX_OF) == 6 and all(len(row) == 16 for row in g.PIX_OF)
    flat = [p for row in g.PIX_OF for p in row]
    assert sorted(p for p in flat if p != g.PAD) == list(range(RANKS * FILES))
    assert flat.count(g.PAD) == 6 and g.PAD < 0
    # the pads sit in the tile whose store address the body keeps apart (V_SBW5)
    assert all(p != g.PAD for row in g.PIX_OF[:5] for p in row)
    # the LDS row swizzle is chunk ^ (p & 7) and the lane table derives it from the column: they must agree, which also
    # keeps each 16-lane group of a fragment read ({0-3, 12-15}, {4-11}) and each 8-lane group of a store on 8 distinct chunks
    assert all(p == g.PAD or p & 7 == c & 7 for row in g.PIX_OF for c, p in enumerate(row))


def test_dead_pairs_are_exactly_the_all_padding_ones():
    import gen_tower1wa as g
    dead = {(n, tap) for n in range(6) for tap in range(9) if not any(_valid(p, tap) for p in g.PIX_OF[n])}
    assert set(g.DEAD) == dead
    for (n, tap) in g.DEAD:
        assert all(not _valid(p, tap) for p in g.PIX_OF[n])
    # what the issue of this change set out to get: the three left taps of the file-0 tile (tile 5), one tap of another tile (not 0)
    assert {(5, 0), (5, 3), (5, 6)} <= dead and len(dead) == 4 and all(n != 0 for n, _ in dead)
    # the schedule leaves out dead pairs only
    assert set(g.SKIP) <= dead
    # of the 810 tap-pixel products 700 are valid; the dead pairs hold none of them
    assert sum(_valid(p, tap) for p in range(90) for tap in range(9)) == 700


def test_stream_has_the_full_count_minus_the_left_out_pairs():
    import gen_tower1wa as g
    lin = _linear(g)
    assert g.check_and_fill(lin, 3)
    per_layer = {}
    for x in lin:
        if x.kind == "mfma" and x.m["want"][0] != "skip":
            per_layer[x.m["want"][0]] = per_layer.get(x.m["want"][0], 0) + 1
    assert sorted(per_layer) == list(range(6))
    assert len(g.SKIP) > 0
    for layer, count in per_layer.items():
        assert count == 1728 - 32 * len(g.SKIP), (layer, count)
    # every (tile, tap, ks) that is not left out is there exactly once per layer, and no left-out one
    seen = {}
    for x in lin:
        if x.kind == "mfma" and x.m["want"][0] != "skip":
            key = (x.m["want"][0], x.m["tile"], x.m["want"][1], x.m["want"][2])
            seen[key] = seen.get(key, 0) + 1
    want = {(layer, t, tap, ks) for layer in range(6) for t in range(48) for tap in range(9) for ks in range(4)
            if (t % 6, tap) not in g.SKIP}
    assert set(seen) == want and set(seen.values()) == {1}


def test_the_checker_notices_one_mfma_too_few_or_too_many():
    import copy
    import gen_tower1wa as g
    n, tap = sorted(g.SKIP)[0]

    def drop_live(l):
        # a live MFMA of the tile that has dead taps, in a live tap
        live_tap = next(t for t in range(1, 8) if (n, t) not in g.SKIP)
        i = next(i for i, x in enumerate(l) if x.kind == "mfma" and x.m["tile"] == g.TILE(3, n) and x.m["want"] == (2, live_tap, 1))
        del l[i]

    def readd_dead(l):
        # the dead pair's MFMA with the operands its neighbour tile's MFMA of the same K-step has: in (tap, ks) order for its
        # accumulator, fragments loaded and waited for - wrong only in that the schedule says its pair is left out
        i = next(i for i, x in enumerate(l) if x.kind == "mfma" and x.m["tile"] == g.TILE(3, n - 1) and x.m["want"] == (2, tap, 0))
        ins = copy.copy(l[i])
        ins.m = dict(ins.m, tile=g.TILE(3, n))
        l.insert(i + 1, ins)

    for mut in (drop_live, readd_dead):
        lin = _linear(g)
        mut(lin)
        with pytest.raises(g.CheckError):
            g.check_and_fill(lin, 3)
