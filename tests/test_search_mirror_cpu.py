"""CPU tests of tests/search_mirror.py: the Python restatement of the search is compared with the pinned oracle's
search_tree node by node before any GPU test trusts it, and the conditions the GPU edge tests rest on (how deep the peaked
evaluator drives a 64-round search and a reused tree) are asserted on the reference side alone."""
import numpy as np
import pytest

from oracle import xq_oracle as xo
from tests import search_mirror as sm


def _start():
    oe = xo.OracleEnv()
    oe.reset()
    return oe


def _same_tree(ref, root, what):
    """visit counts, value_sum bits, prior bits, moves and child ranges of every node, in child order"""
    a, b = sm.flatten_arrays(ref), sm.flatten_nodes(root)
    assert len(a) == len(b) == len(ref["move"]), (what, len(a), len(b))
    for x, y in zip(a, b):
        assert x == y, (what, x, y)


@pytest.fixture(scope="module")
def peaked():
    return sm.peaked_oracle_evaluator()


@pytest.fixture(scope="module")
def tree512(peaked):
    return _start().search_tree(512, peaked)


def test_peaked_evaluator_is_the_same_function_behind_both_wrappers(peaked):
    """the oracle callback and the predict_batch object hand out the same fp32 priors and fp64 value for a position;
    the priors are the peak on one move and an even share elsewhere, the value a multiple of 1/256 in [-2, 2]/256"""
    from chinesechessai_amd.chess_env import decode_move
    oe = _start()
    legal = oe.legal_moves()
    b = oe.board().reshape(90)
    idx, val = sm.peaked_eval(b, 1, len(legal))
    probs, v = sm.PeakedNet().predict_batch([(oe.board(), 1, [decode_move(m) for m in legal])])[0]
    got = np.array([probs[decode_move(m)] for m in legal], dtype=np.float32)
    exp = sm.peaked_priors(len(legal), idx)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32)) and v == val
    assert exp[idx] == np.float32(0.97) and (np.delete(exp, idx) == np.float32(0.03 / (len(legal) - 1))).all()
    assert val * 256 == int(val * 256) and abs(val) <= 2 / 256
    ref = oe.search_tree(9, peaked)                        # one expansion below the root: its children carry the priors
    f = int(ref["first_child"][0])
    assert np.array_equal(ref["prior"][f:f + len(legal)].view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("sims", [15, 50, 512])
def test_mirror_equals_oracle_with_the_peaked_evaluator(peaked, tree512, sims):
    oe = _start()
    ref = tree512 if sims == 512 else oe.search_tree(sims, peaked)
    moves, counts, root = sm.search_mirror(oe, sm.Node(), sims)
    _same_tree(ref, root, sims)
    f, n = int(ref["first_child"][0]), int(ref["n_child"][0])
    assert moves == ref["move"][f:f + n].tolist() and counts == ref["visit_count"][f:f + n].tolist()
    assert int(ref["visit_count"][0]) == sims


@pytest.mark.parametrize("k", [2, 5, 9])
def test_mirror_equals_oracle_with_hashnet_on_seeded_positions(k):
    envs, lines = sm.seeded_positions()
    oe = envs[k]
    assert len(lines[k]) == 3 * k
    ref = oe.search_tree(50)
    _, _, root = sm.search_mirror(oe, sm.Node(), 50, evaluate=sm.hashnet_evaluate)
    _same_tree(ref, root, k)


def test_sixty_four_rounds_reach_level_63_and_no_deeper(tree512):
    """what the GPU 64-round test rests on: 512 simulations of the peaked search from the start position visit a node
    on level 63 (the last level a 64-lane backup serves) and none below; 504 stop one level short"""
    flat = sm.flatten_arrays(tree512)
    assert max(sm.visited_depths(flat)) == 63
    assert max(t[0] for t in flat) == 64                   # (created, never visited)
    flat504 = sm.flatten_arrays(_start().search_tree(504, sm.peaked_oracle_evaluator()))
    assert max(sm.visited_depths(flat504)) == 62


@pytest.mark.parametrize("virtual_loss", [False, True])
def test_reused_trees_grow_past_level_64_at_ply_2(virtual_loss):
    """what the GPU reuse tests rest on: S = 200, tree reuse, argmax play from the start position - the tree searched at
    ply 2 has at least three visited nodes on level 64 or deeper, the tree of ply 1 none; no path passes level 70 (the
    rules end a game at move_count >= 70); every ply keeps the played child's subtree"""
    plies = sm.play_reuse_mirror(200, 4, virtual_loss=virtual_loss)
    deep = [sum(1 for d in sm.visited_depths(p["flat"]) if d >= 64) for p in plies]
    top = [max(sm.visited_depths(p["flat"])) for p in plies]
    print("deepest visited level per ply %s, visited nodes on level >= 64 per ply %s" % (top, deep))
    assert deep[0] == 0 and deep[1] == 0 and deep[2] >= 3, (deep, top)
    assert all(ply + t <= 70 for ply, t in enumerate(top)), top
    assert plies[0]["root_idx"] == 0 and all(p["root_idx"] != 0 for p in plies[1:])
    for p in plies:
        assert p["played"] == p["moves"][int(np.argmax(p["counts"]))]
