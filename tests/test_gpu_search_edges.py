"""GPU tests (`-m gpu`, through the C ABI) of three search states the rest of the suite never reaches: the 64-round limit
(paths 63 levels deep), reused trees whose paths pass level 64, and roots with stale king caches under the evaluation
cache.  The references are the CPU oracle and tests/search_mirror.py (validated against the oracle by
tests/test_search_mirror_cpu.py); every comparison is bit-exact.  One evaluator - search_mirror.peaked_eval, the stand-in
for a trained (peaked) network - drives the engine and the references."""
import json
import os

import numpy as np
import pytest

from tests import search_mirror as sm

pytestmark = pytest.mark.gpu

NG = 4


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


def _state_rows(envs):
    """(boards [n][90], state rows) of oracle envs for xq_engine_set_roots"""
    from chinesechessai_amd import _lib
    boards = np.stack([np.array(oe.board(), dtype=np.int8).reshape(90) for oe in envs])
    st = np.zeros((len(envs), _lib.STATE_WORDS), np.int32)
    for i, oe in enumerate(envs):
        e = oe.e
        st[i, _lib.S_PLAYER], st[i, _lib.S_MOVE_COUNT], st[i, _lib.S_WINNER] = e.current_player, e.move_count, _lib.WINNER_NONE
        st[i, _lib.S_RED_KING], st[i, _lib.S_BLACK_KING], st[i, _lib.S_NO_CAPTURE] = e.red_king, e.black_king, e.no_capture_count
    return boards, st


def test_sixty_four_rounds_equal_the_oracle_node_by_node(L):
    """sims = 512 = 64 rounds of 8, the most xq_engine_create accepts: with the peaked evaluator the search follows one line
    and its last rounds back up paths 63 levels deep (lane 63 of the lane-per-level code).  Game g starts from the start
    position after g seeded random plies; every node of every tree - visit_count, value_sum bits, prior bits, move, child
    range - equals OracleEnv.search_tree(512).  One round more is refused when the engine is created."""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import CallbackEvaluator, SelfPlayEngine
    S = 512
    envs, lines = sm.seeded_positions(seed=20261020, count=NG, step=1)
    assert len(envs) == NG and [len(x) for x in lines] == list(range(NG))
    boards, st = _state_rows(envs)
    eng = SelfPlayEngine(NG, sims=S)
    assert eng.rounds == 64
    ev = CallbackEvaluator(sm.PeakedNet())
    ev.bind(eng)
    eng.set_roots(boards, st)
    eng.search(ev)
    peaked = sm.peaked_oracle_evaluator()
    total, deepest = 0, []
    for i, oe in enumerate(envs):
        ref = oe.search_tree(S, peaked)
        got = eng.read_tree(i)
        m = len(ref["move"])
        deepest.append(max(sm.visited_depths(sm.flatten_arrays(ref))))
        assert got["root"] == 0 and len(got["move"]) == m, (i, len(got["move"]), m)
        assert np.array_equal(got["visit_count"].astype(np.int64), ref["visit_count"]), i
        assert np.array_equal(got["value_sum"].view(np.uint64), ref["value_sum"].view(np.uint64)), i
        assert np.array_equal(got["prior"][1:].view(np.uint32), ref["prior"][1:].view(np.uint32)), i
        assert np.array_equal(got["move"][1:], ref["move"][1:]), i
        assert np.array_equal(got["n_child"].astype(np.int64), ref["n_child"]), i
        exp = ref["n_child"] > 0
        assert np.array_equal(got["first_child"].astype(np.int64)[exp], ref["first_child"][exp]), i
        assert int(ref["visit_count"][0]) == S
        total += m
    eng.close()
    assert deepest[0] == 63, deepest                       # the start position: the level the limit exists for is reached
    print("64-round trees compared node by node with the oracle's: %d nodes, deepest visited level per game %s" % (total, deepest))
    with pytest.raises(_lib.XqError, match="at most 64 rounds per move"):
        SelfPlayEngine(NG, sims=S + 1)


class PlanesPeakedEvaluator:
    """peaked_eval for engines with several pending leaves per game (virtual loss), where the host-callback path
    (xq_engine_read_leaves) is refused: the search kernel writes each pending leaf's float32 input planes, this evaluator
    decodes board and side to move from them, asks the rules oracle for the legal moves (play from the start position keeps
    the king caches true, so the position fixes the list) and hands the priors in by slot (XQ_EVAL_PRIORS) from its own
    device buffers.  Slots without a pending leaf hold an older leaf's planes; their rows are computed and ignored."""
    deterministic = True

    def __init__(self):
        from chinesechessai_amd import _lib
        self.planes_format = _lib.PLANES_NCHW_F32
        self.memo, self.by_planes = {}, {}

    def bind(self, engine):
        import torch
        n = engine.n_rows
        self.storage = torch.zeros((n, 15, 90), dtype=torch.float32, device="cuda")
        self.priors = torch.zeros((n, 128), dtype=torch.float32, device="cuda")
        self.values = torch.zeros((n,), dtype=torch.float64, device="cuda")

    def planes_ptr(self):
        return self.storage.data_ptr()

    def _row(self, planes):
        from oracle import xq_oracle as xo
        board = np.zeros(90, np.int8)
        for c in range(14):
            board[planes[c] != 0] = c + 1 if c < 7 else -(c - 6)
        side = 1 if planes[14, 0] != 0 else -1
        key = (board.tobytes(), side)
        if key not in self.memo:
            rk, bk = np.where(board == 1)[0], np.where(board == -1)[0]
            oe = xo.OracleEnv()
            oe.set_state(board, side, red_king=int(rk[0]) if len(rk) else xo.NO_KING,
                         black_king=int(bk[0]) if len(bk) else xo.NO_KING)
            n = len(oe.legal_moves())
            p = np.zeros(128, np.float32)
            val = 0.0
            if n:
                idx, val = sm.peaked_eval(board, side, n)
                p[:n] = sm.peaked_priors(n, idx)
            self.memo[key] = (p, val)
        return self.memo[key]

    def evaluate(self, engine):
        import torch
        from chinesechessai_amd import _lib
        planes = self.storage.cpu().numpy()                 # (the default stream: ordered behind the search kernel)
        pri = np.zeros((len(planes), 128), np.float32)
        val = np.zeros(len(planes), np.float64)
        for s in range(len(planes)):
            raw = planes[s].tobytes()
            if raw not in self.by_planes:
                self.by_planes[raw] = self._row(planes[s]) if planes[s, :14].any() else (pri[s], 0.0)
            pri[s], val[s] = self.by_planes[raw]
        self.priors.copy_(torch.from_numpy(pri))
        self.values.copy_(torch.from_numpy(val))
        torch.cuda.synchronize()
        return _lib.EVAL_PRIORS, self.priors.data_ptr(), self.values.data_ptr()


_MIRROR = {}


def _mirror_plies(virtual_loss):
    if virtual_loss not in _MIRROR:
        _MIRROR[virtual_loss] = sm.play_reuse_mirror(200, 4, virtual_loss=virtual_loss)
    return _MIRROR[virtual_loss]


def _reused_trees(virtual_loss):
    """sims = 200, tree reuse, argmax play, four plies stepped by hand from the start position: per ply the subtree below
    the engine's root, walked in child order, against the mirror's tree - move, N, W bits, P bits, child count and the
    index of the first child (the mirror numbers its nodes as the arena does) - then the played moves and the stored
    visit counts.  The four games are the same game (one start position, argmax play): game 0 is walked, the arenas of
    the others must equal game 0's array by array.  Returns ({ply: first difference}, report)."""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import CallbackEvaluator, SelfPlayEngine
    S, PLIES = 200, 4
    ref = _mirror_plies(virtual_loss)
    deep = [sum(1 for d in sm.visited_depths(p["flat"]) if d >= 64) for p in ref]
    assert deep[0] == 0 and deep[1] == 0 and deep[2] >= 3, deep           # (what test_search_mirror_cpu.py pins)
    # max_moves = 8: the arena holds eight plies of expansions, so the "does a whole ply still fit" rule never drops a tree
    eng = SelfPlayEngine(NG, sims=S, temperature=0.0, max_moves=8,
                         planes_format=_lib.PLANES_NCHW_F32 if virtual_loss else _lib.PLANES_NONE)
    eng.set_tree_reuse(True)
    if virtual_loss:
        eng.set_virtual_loss(True)
        ev = PlanesPeakedEvaluator()
    else:
        ev = CallbackEvaluator(sm.PeakedNet())
    ev.bind(eng)
    eng.new_games(np.arange(NG, dtype=np.uint32))
    bad, sizes = {}, []
    for ply in range(PLIES):
        eng.search(ev)
        for g in range(NG):
            t = eng.read_tree(g)
            assert (t["root"] != 0) == (ply > 0), (ply, g, t["root"])
            assert t["root"] == ref[ply]["root_idx"], (ply, g, t["root"], ref[ply]["root_idx"])
            if g > 0:
                for k in ("visit_count", "value_sum", "prior", "move", "first_child", "n_child"):
                    if ply not in bad and t[k].tobytes() != t0[k].tobytes():
                        bad[ply] = "game %d: %s differs from game 0's" % (g, k)
                continue
            t0 = t
            got, exp = sm.flatten_arrays(t, t["root"]), ref[ply]["flat"]
            if ply not in bad:
                if len(got) != len(exp):
                    bad[ply] = "game %d: %d nodes below the root, the mirror has %d" % (g, len(got), len(exp))
                else:
                    for k, (x, y) in enumerate(zip(got, exp)):
                        if x != y:
                            bad[ply] = ("game %d, node %d in child order (level, move, N, W bits, P bits, children, first child): "
                                        "engine %s, mirror %s" % (g, k, x, y))
                            break
            sizes.append(len(got))
        _lib.check(eng.L.xq_engine_play_move(eng.h))
    _lib.check(eng.L.xq_engine_finalize(eng.h))
    b = eng.read_results()
    if virtual_loss:
        assert (eng.tree_stats()[1] == 0).all()
    eng.close()
    for ply in range(PLIES):
        if ply in bad:
            continue
        n = len(ref[ply]["moves"])
        for g in range(NG):
            if int(b.chosen[g, ply]) != ref[ply]["played"]:
                bad[ply] = "game %d played %d, the mirror %d" % (g, int(b.chosen[g, ply]), ref[ply]["played"])
            elif int(b.s_n[g, ply]) != n or b.s_moves[g, ply, :n].tolist() != ref[ply]["moves"] or \
                    b.s_counts[g, ply, :n].tolist() != ref[ply]["counts"]:
                bad[ply] = "game %d: stored root visits differ from the mirror's" % g
    assert (b.n_plies == PLIES).all() and int(b.error.sum()) == 0
    report = "reused trees%s: nodes below the root per ply %s, visited nodes on level >= 64 per ply %s" % (
        " with virtual loss" if virtual_loss else "", sizes, deep)
    return bad, report


def test_reused_trees_equal_the_mirror_node_by_node(L):
    """Tree reuse keeps the played child's subtree with its depth: at S = 200 with peaked priors the tree searched at ply 2
    has visited nodes down to level 68 (a game ends at move_count >= 70, so no path is longer than 70 - ply levels).  Every
    level must be backed up: each ply's tree equals the mirror's node by node (k_search_round's one-leaf form)."""
    bad, report = _reused_trees(False)
    print(report)
    assert not bad, "\n".join("ply %d: %s" % kv for kv in sorted(bad.items()))


def test_reused_trees_with_virtual_loss_equal_the_mirror_node_by_node(L):
    """The same with virtual loss: eight pending leaves per game and round (search_round_generic, consume_eval and the
    pending-visit counters of every level of a path); the mirror reaches level 68 at ply 2 here too."""
    bad, report = _reused_trees(True)
    print(report)
    assert not bad, "\n".join("ply %d: %s" % kv for kv in sorted(bad.items()))


def _edge_case(golden_dir, name):
    with open(os.path.join(golden_dir, "rules_edge.json")) as f:
        return next(c for c in json.load(f) if c["name"] == name)


def _true_kings(board):
    from oracle import xq_oracle as xo
    rk, bk = np.where(np.asarray(board).reshape(90) == 1)[0], np.where(np.asarray(board).reshape(90) == -1)[0]
    return (int(rk[0]) if len(rk) else xo.NO_KING, int(bk[0]) if len(bk) else xo.NO_KING)


def test_stale_king_caches_do_not_reach_the_evaluation_cache(L, golden_dir):
    """The evaluation cache is keyed by board + side; its priors are indexed by the leaf's legal-move list, which also depends
    on the two king caches - and xq_engine_set_roots accepts any caches (the reference's own unit boards carry stale ones).
    P = the edge board `no_king_cache` (the red king stands on the board, its cache says NO_KING); game B plays a move m
    from P to Q and carries the stale cache along; game A of the same engine starts at Q with true caches and fills Q's
    cache entry at ply 0; at ply 1 game B's root is Q, inside the cache's two-ply window, with another legal-move list
    (asserted with the oracle).  Required: both games' records equal their own cache-less runs, with the cache on and in
    verify mode, and verify mode finds no mismatch.  The engine achieves that by keeping the cache off while any root of
    xq_engine_set_roots carries a stale king cache (its statistics stay at 0); consistent roots switch it on again."""
    import torch
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    from oracle import xq_oracle as xo
    S = 48
    c = _edge_case(golden_dir, "no_king_cache")
    assert (c["red_king"], c["black_king"]) != _true_kings(c["board"])    # stale as the case sets it
    torch.manual_seed(11)
    net = ChessNet(num_blocks=2).eval().cuda()
    inet = []

    def root_row(board, player, move_count, rk, bk, nocap):
        st = np.zeros(_lib.STATE_WORDS, np.int32)
        st[_lib.S_PLAYER], st[_lib.S_MOVE_COUNT], st[_lib.S_WINNER] = player, move_count, _lib.WINNER_NONE
        st[_lib.S_RED_KING], st[_lib.S_BLACK_KING], st[_lib.S_NO_CAPTURE] = rk, bk, nocap
        return np.asarray(board, np.int8).reshape(90), st

    def run(roots, uniforms, cache, again=None):
        ev = TorchNetEvaluator(inet[0] if inet else net, leaf_dedupe=False, eval_cache=cache)
        if not inet:
            inet.append(ev.inet)
        n = len(roots)
        eng = SelfPlayEngine(n, sims=S, planes_format=ev.planes_format, max_moves=2)
        eng.set_root_eval_carry(False)
        ev.bind(eng)
        assert eng.eval_cache == bool(cache) and not eng.leaf_dedupe

        def two_plies(rts, us):
            eng.set_roots(np.stack([r[0] for r in rts]), np.stack([r[1] for r in rts]))
            u = np.zeros((n, _lib.MAX_PLIES))
            u[:, :2] = np.asarray(us).reshape(n, 2)
            eng.set_uniforms(u)
            for _ in range(2):
                eng.search(ev)
                _lib.check(eng.L.xq_engine_play_move(eng.h))
            _lib.check(eng.L.xq_engine_finalize(eng.h))
            return eng.read_results(), (eng.eval_cache_stats(reset=True) if cache else (0, 0, 0))
        out = two_plies(roots, uniforms)
        if again is not None:
            out = out + two_plies(again, [[0.5, 0.5]] * n)
        eng.close()
        return out

    def same(a, ga, b, gb, what):
        assert int(a.error[ga]) == 0 and int(b.error[gb]) == 0, what
        for k in ("n_plies", "n_samples", "winner", "reason"):
            assert int(getattr(a, k)[ga]) == int(getattr(b, k)[gb]), (what, k)
        for k in ("chosen", "s_n", "s_moves", "s_counts", "s_player"):
            assert np.array_equal(getattr(a, k)[ga, :2], getattr(b, k)[gb, :2]), (what, k)

    rootP = root_row(c["board"], c["player"], 0, c["red_king"], c["black_king"], 0)
    # game B alone, cache off: its reference records, and the move m it plays at ply 0 (the uniform of ply 0 is varied until
    # m leads to a Q whose legal-move list depends on the carried cache: 15 of P's 19 moves do)
    found = None
    for u0 in (0.1, 0.3, 0.5, 0.7, 0.9):
        refB, _ = run([rootP], [[u0, 0.5]], False)
        m = int(refB.chosen[0, 0])
        oe = xo.OracleEnv()
        oe.set_state(c["board"], c["player"], red_king=c["red_king"], black_king=c["black_king"])
        assert m in oe.legal_moves()
        _, done, _ = oe.make_move(m)
        carried = oe.legal_moves()
        rk, bk = _true_kings(oe.board())
        ot = xo.OracleEnv()
        ot.set_state(oe.board(), oe.e.current_player, move_count=oe.e.move_count, red_king=rk, black_king=bk,
                     no_capture=oe.e.no_capture_count)
        true = ot.legal_moves()
        if not done and carried and true and carried != true and (oe.e.red_king, oe.e.black_king) != (rk, bk):
            found = (u0, oe, ot, carried, true)
            break
    assert found is not None, "no ply-0 move of game B leads to a position whose legal moves depend on the stale cache"
    u0, oe, ot, carried, true = found
    assert carried != true and int(refB.n_plies[0]) == 2
    assert refB.s_moves[0, 1, :int(refB.s_n[0, 1])].tolist() == carried           # B's ply-1 root: Q with the carried caches
    rootQ = root_row(ot.board(), ot.e.current_player, ot.e.move_count, ot.e.red_king, ot.e.black_king, ot.e.no_capture_count)
    refA, _ = run([rootQ], [[0.5, 0.5]], False)
    assert refA.s_moves[0, 0, :int(refA.s_n[0, 0])].tolist() == true              # A's root: Q with true caches
    uAB = [[0.5, 0.5], [u0, 0.5]]
    for mode in ("verify", "on"):
        both, stats, clean, stats_clean = run([rootQ, rootP], uAB, mode, again=[rootQ, rootQ])
        print("eval cache %s, games A (Q, true caches) + B (P -> Q, stale red-king cache): hits / fills / mismatches %s; "
              "after consistent roots %s" % (mode, stats, stats_clean))
        assert stats[2] == 0, (mode, stats)
        same(both, 0, refA, 0, (mode, "A"))
        same(both, 1, refB, 0, (mode, "B"))
        assert stats == (0, 0, 0), (mode, stats)             # off while a root's king cache is stale ...
        assert stats_clean[1] > 0 and stats_clean[2] == 0, (mode, stats_clean)    # ... and on again with consistent roots
        same(clean, 0, refA, 0, (mode, "A again"))
        same(clean, 1, refA, 0, (mode, "A twice"))
