"""CPU tests of tests/wide_positions.py and of what tests/test_gpu_wide_nodes.py rests on: the boards are what they are
declared to be, the mirror equals the pinned oracle on them, and the oracle's trees really reach the upper half (children
64..127) of wide nodes, so the GPU comparisons cannot pass without running that half."""
import numpy as np
import pytest

from oracle import xq_oracle as xo
from tests import search_mirror as sm
from tests import wide_positions as wp

SIMS = (50, 200)
EVALUATORS = ("hashnet", "peaked", "uniform")


def test_the_list_holds_the_widths_it_must():
    widths = {b[0]: b[1] for b in wp.BOARDS}
    assert 64 in widths.values() and 65 in widths.values() and 128 in widths.values()
    assert 70 <= widths["lawful_both"] <= 80 and any(100 <= w <= 127 for w in widths.values())
    assert "many_moves" in widths and max(widths.values()) <= wp.MAX_CANDIDATES
    both = [b for b in wp.BOARDS if b[0] in wp.BOTH_WIDE]
    assert len(both) >= 2 and all(b[1] > 64 and b[2] > 64 for b in both)
    assert {b[4] for b in both} == {1, -1}                     # a wide red root and a wide black root
    # lawful material: what the start position holds, on both sides
    for name in ("lawful_both", "lawful_both_black"):
        b = wp.board90(name)
        for side in (1, -1):
            assert [int((b == side * p).sum()) for p in range(1, 8)] == [1, 2, 2, 2, 2, 2, 5], (name, side)


def test_many_moves_is_the_edge_board_of_the_golden_file(golden_dir):
    import json
    import os
    with open(os.path.join(golden_dir, "rules_edge.json")) as f:
        c = next(x for x in json.load(f) if x["name"] == "many_moves")
    _, width, _, _, side, rk, bk = wp.entry("many_moves")
    assert c["board"] == wp.board90("many_moves").tolist() and c["player"] == side
    assert (c["red_king"], c["black_king"]) == (xo.sq(rk), xo.sq(bk)) and len(c["legal"]) == width
    assert c["legal"] == wp.env_of("many_moves").legal_moves()


@pytest.mark.parametrize("name", wp.ALL_NAMES)
def test_board_is_what_it_is_declared_to_be(name):
    """width by the oracle; no listed move suicidal, and no pseudo-legal move at all (pseudo-legal count == width <= 128);
    true king caches, kings in their palaces; advisors, bishops and pawns on lawful squares; nobody in check except the
    bare black king of `many_moves` (it is not to move); every move has a column in both policy layouts"""
    from chinesechessai_amd.neural_network import reachable_policy_columns
    _, width, other, pieces, side, rk, bk = wp.entry(name)
    b = wp.board90(name)
    oe = wp.env_of(name)
    moves = oe.legal_moves()
    assert len(moves) == width and len(set(moves)) == width
    assert wp.raw_counts(oe) == (width, width) and width <= wp.MAX_CANDIDATES
    assert not any(oe.is_move_suicide(m) for m in moves)
    assert wp.raw_counts(wp.env_of(name, -side))[0] == other
    assert not xo.lib().xqo_is_in_check(oe.p, side)
    if name != "many_moves":
        assert not xo.lib().xqo_is_in_check(wp.env_of(name, -side).p, -side)
    # kings
    assert np.where(b == 1)[0].tolist() == [xo.sq(rk)] and np.where(b == -1)[0].tolist() == [xo.sq(bk)]
    assert 7 <= rk[0] <= 9 and 3 <= rk[1] <= 5 and 0 <= bk[0] <= 2 and 3 <= bk[1] <= 5
    # lawful squares (red's; black's mirrored top to bottom)
    adv = {(7, 3), (7, 5), (8, 4), (9, 3), (9, 5)}
    bis = {(9, 2), (9, 6), (7, 0), (7, 4), (7, 8), (5, 2), (5, 6)}
    for (r, c), p in pieces.items():
        rr = r if p > 0 else 9 - r
        if abs(p) == wp.A:
            assert (rr, c) in adv, (name, r, c)
        elif abs(p) == wp.B:
            assert (rr, c) in bis, (name, r, c)
        elif abs(p) == wp.Pw:
            assert rr <= 4 or (rr <= 6 and c % 2 == 0), (name, r, c)
    assert max(int((b > 0).sum()), int((b < 0).sum())) <= 16
    # policy columns: the compact (reachable) map and the full 8,100-column layout
    cols, cmap = reachable_policy_columns()
    mv = np.asarray(moves)
    assert (cmap[mv] >= 0).all() and len(set(cmap[mv].tolist())) == width
    # the full layout (policy_columns="all") has no map to miss: column = move index, so the bound is the whole condition
    assert 0 <= mv.min() and mv.max() < 8100
    # the other side's moves too (depth-1 nodes)
    assert (cmap[np.asarray(wp.env_of(name, -side).legal_moves(), dtype=np.int64)] >= 0).all()


def _same_tree(ref, root, what):
    a, b = sm.flatten_arrays(ref), sm.flatten_nodes(root)
    assert len(a) == len(b) == len(ref["move"]), (what, len(a), len(b))
    for x, y in zip(a, b):
        assert x == y, (what, x, y)


@pytest.mark.parametrize("evaluator", EVALUATORS)
@pytest.mark.parametrize("name", wp.ALL_NAMES)
def test_mirror_without_virtual_loss_equals_the_oracle_node_by_node(name, evaluator):
    oe = wp.env_of(name)
    for sims in SIMS:
        ref = wp.oracle_tree(name, sims, evaluator)
        moves, counts, root = sm.search_mirror(oe, sm.Node(), sims, evaluate=wp.evaluators()[evaluator][1])
        _same_tree(ref, root, (name, evaluator, sims))
        f, n = int(ref["first_child"][0]), int(ref["n_child"][0])
        assert n == wp.entry(name)[1] and int(ref["visit_count"][0]) == sims
        assert moves == ref["move"][f:f + n].tolist() and counts == ref["visit_count"][f:f + n].tolist()


def test_uniform_evaluator_is_the_same_function_behind_its_three_wrappers():
    from chinesechessai_amd.chess_env import decode_move
    oe = wp.env_of("w65")
    legal = oe.legal_moves()
    exp = np.full(65, np.float32(1) / np.float32(65), np.float32)
    pri, val = sm.uniform_evaluate(oe.board().reshape(90), 1, legal)
    assert val == 0.0 and np.array_equal(np.asarray(pri, np.float32).view(np.uint32), exp.view(np.uint32))
    probs, v = sm.UniformNet().predict_batch([(oe.board(), 1, [decode_move(m) for m in legal])])[0]
    assert v == 0.0 and all(probs[decode_move(m)].view(np.uint32) == exp[0].view(np.uint32) for m in legal)
    ref = wp.oracle_tree("w65", 50, "uniform")
    f = int(ref["first_child"][0])
    assert np.array_equal(ref["prior"][f:f + 65].view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("evaluator", EVALUATORS)
def test_every_expanded_node_stays_within_the_candidate_cap(evaluator):
    """the device keeps 128 pseudo-legal candidates per node: every node the oracle expands in the trees the tests compare
    has at most that many (legal ones equal to its child count), so no compared tree leaves the contract"""
    worst = 0
    for name in wp.ALL_NAMES:
        for sims in SIMS:
            tree = wp.oracle_tree(name, sims, evaluator)
            for i, oe in wp.node_envs(name, tree):
                legal, pseudo = wp.raw_counts(oe)
                assert legal == tree["n_child"][i] and pseudo <= wp.MAX_CANDIDATES, (name, sims, i, legal, pseudo)
                worst = max(worst, pseudo)
    print("%s: most pseudo-legal moves at an expanded node %d" % (evaluator, worst))


@pytest.mark.parametrize("sims", [24, 200])
def test_every_node_the_virtual_loss_mirror_expands_stays_within_the_candidate_cap(sims):
    """the same for the trees the generic-kernel test compares: search_mirror(virtual_loss=True) with the peaked evaluator
    from every board, `w128` included - its widest expanded node is the 128-child root itself"""
    worst = {name: wp.mirror_max_candidates(name, wp.vl_mirror(name, sims)) for name in wp.ALL_NAMES}
    print("virtual-loss mirror, S = %d: most pseudo-legal moves at an expanded node %s" % (sims, worst))
    assert max(worst.values()) <= wp.MAX_CANDIDATES and worst["w128"] == 128, worst


@pytest.mark.parametrize("salt", [0, 1])
def test_two_network_reference_trees_from_the_cap_board_stay_within_the_cap(salt):
    """the HashNet S = 50 trees of the two-network test from `w128` (either salt)"""
    from tests.test_oracle_search import _salted
    oe = wp.env_of("w128")
    assert wp.max_candidates(oe, oe.search_tree(50, _salted(salt) if salt else None)) <= wp.MAX_CANDIDATES


def _coverage(evaluator):
    """over the oracle's trees of one evaluator: (trees with an expanded, visited root child of index >= 64; trees with a
    non-root node of more than 64 children; trees where the most visited child of some node wider than 64 has index >= 64)"""
    upper, nonroot, best = [], [], []
    for name in wp.ALL_NAMES:
        for sims in SIMS:
            t = wp.oracle_tree(name, sims, evaluator)
            f, n = int(t["first_child"][0]), int(t["n_child"][0])
            if any(t["visit_count"][f + j] > 0 and t["n_child"][f + j] > 0 for j in range(64, n)):
                upper.append((name, sims))
            if (t["n_child"][1:] > 64).any():
                nonroot.append((name, sims))
            for i in np.where(t["n_child"] > 64)[0]:
                ff, k = int(t["first_child"][i]), int(t["n_child"][i])
                v = t["visit_count"][ff:ff + k]
                if v.max() > 0 and int(np.argmax(v)) >= 64:
                    best.append((name, sims))
                    break
    return upper, nonroot, best


def test_hashnet_trees_reach_the_upper_half():
    upper, nonroot, _ = _coverage("hashnet")
    assert upper and nonroot, (upper, nonroot)
    assert {n for n, _ in nonroot} >= set(wp.BOTH_WIDE)


def test_peaked_trees_reach_the_upper_half_and_prefer_it_somewhere():
    upper, nonroot, best = _coverage("peaked")
    assert upper and nonroot and best, (upper, nonroot, best)


def test_uniform_trees_reach_wide_nodes_below_the_root_and_stop_short_of_child_64():
    """With equal priors and value 0 a visited child scores 1.5 P sqrt(N) / (1 + n) with n >= 1, an unvisited one twice
    that or more, so the search expands the root's children strictly in index order, one per round of 8 simulations:
    child 64 would take 66 rounds, and 64 (512 simulations) are the most an engine accepts.  An expanded root child of
    index >= 64 therefore cannot exist for this evaluator at any size the engine runs; what it is here for is the tie:
    at every wide node all unvisited children - the upper half among them - score the same float32, and the first index
    must win.  Asserted: wide nodes below the root exist, and in every tree the visited children of every wide node are
    exactly its first ones (a tie-break that let a lane of the upper half win would break that)."""
    upper, nonroot, _ = _coverage("uniform")
    assert not upper and nonroot, (upper, nonroot)
    assert {n for n, _ in nonroot} >= set(wp.BOTH_WIDE)
    seen = 0
    for name in wp.ALL_NAMES:
        for sims in SIMS:
            t = wp.oracle_tree(name, sims, "uniform")
            for i in np.where(t["n_child"] > 64)[0]:
                ff, k = int(t["first_child"][i]), int(t["n_child"][i])
                v = t["visit_count"][ff:ff + k]
                nz = int((v > 0).sum())
                if i == 0 or name in wp.BOTH_WIDE:              # (no terminal children at these nodes)
                    assert (v[:nz] > 0).all() and (v[nz:] == 0).all(), (name, sims, i)
                    seen += nz > 0
    assert seen >= len(wp.ALL_NAMES)


@pytest.mark.parametrize("virtual_loss", [False, True])
@pytest.mark.parametrize("name", wp.BOTH_WIDE)
def test_reuse_mirror_starts_from_a_given_position_and_keeps_wide_roots(name, virtual_loss):
    """play_reuse_mirror(start_env=...): ply 0 is searched from the board (without virtual loss: the oracle's tree), the
    env handed in is not changed, and on the both-sides-wide boards the roots of the later plies - the played child's kept
    subtree - are wider than 64 too"""
    oe = wp.env_of(name)
    before = bytes(oe.e.board), oe.e.current_player, oe.e.move_count
    plies = sm.play_reuse_mirror(64, 3, virtual_loss=virtual_loss, start_env=oe)
    assert (bytes(oe.e.board), oe.e.current_player, oe.e.move_count) == before
    assert plies[0]["moves"] == oe.legal_moves()
    if not virtual_loss:
        assert plies[0]["flat"] == sm.flatten_arrays(env_tree(oe, 64))
    assert all(len(p["moves"]) > 64 for p in plies), [len(p["moves"]) for p in plies]
    assert plies[0]["root_idx"] == 0 and any(p["root_idx"] != 0 for p in plies[1:])
    for p in plies:
        assert p["played"] == p["moves"][int(np.argmax(p["counts"]))]


def env_tree(oe, sims):
    return oe.search_tree(sims, sm.peaked_oracle_evaluator())
