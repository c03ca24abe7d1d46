"""GPU tests (`-m gpu`, through the C ABI) of search, evaluation and sampling at nodes with more than 64 children: the
second half of every lane-per-child loop (lane l also carries child l + 64) in select_child, consume_eval, the one-leaf
kernel, root_noise, the evaluation cache, k_play_move, pack_samples, read_leaves and write_priors.  The positions are
tests/wide_positions.py; the references are the CPU oracle and tests/search_mirror.py, whose agreement on these positions
and whose reach into the upper half tests/test_wide_nodes_cpu.py asserts.  Tree, record and sampling comparisons are bit
for bit; the softmax and the Dirichlet noise have the bounds their tests state."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import search_mirror as sm
from tests import wide_positions as wp
from tests.test_gpu_round4 import _same_game
from tests.test_gpu_search_edges import PlanesPeakedEvaluator, _state_rows
from tests.test_oracle_search import _salted

pytestmark = pytest.mark.gpu

REP = 4                                                       # slots per board where equality across slots is checked too
TREE_FIELDS = ("visit_count", "value_sum", "prior", "move", "first_child", "n_child")


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


def _roots(names, rep=1):
    """(envs, boards, state rows): every board `rep` times, slot = rep * board + copy"""
    envs = [wp.env_of(n) for n in names for _ in range(rep)]
    boards, st = _state_rows(envs)
    return envs, boards, st


def _equals_oracle_tree(got, ref, ctx):
    m = len(ref["move"])
    assert got["root"] == 0 and len(got["move"]) == m, (ctx, len(got["move"]), m)
    assert np.array_equal(got["visit_count"].astype(np.int64), ref["visit_count"]), ctx
    assert np.array_equal(got["value_sum"].view(np.uint64), ref["value_sum"].view(np.uint64)), ctx
    assert np.array_equal(got["prior"][1:].view(np.uint32), ref["prior"][1:].view(np.uint32)), ctx
    assert np.array_equal(got["move"][1:], ref["move"][1:]), ctx
    assert np.array_equal(got["n_child"].astype(np.int64), ref["n_child"]), ctx
    exp = ref["n_child"] > 0
    assert np.array_equal(got["first_child"].astype(np.int64)[exp], ref["first_child"][exp]), ctx


def _same_as_slot(t, t0, ctx):
    for k in TREE_FIELDS:
        assert t[k].tobytes() == t0[k].tobytes(), (ctx, k)
    assert t["root"] == t0["root"], ctx


def _engine_evaluator(name):
    from chinesechessai_amd.engine import CallbackEvaluator, HashNetEvaluator
    net = wp.evaluators()[name][2]
    return HashNetEvaluator() if net is None else CallbackEvaluator(net())


# ---- a: the one-leaf kernel against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("evaluator", ["hashnet", "peaked", "uniform"])
@pytest.mark.parametrize("sims", [50, 200])
def test_one_leaf_kernel_equals_the_oracle_at_wide_roots(L, sims, evaluator):
    """xq_engine_set_roots on every wide board (4 slots each), one search: every node of every tree - visit_count,
    value_sum bits, prior bits, move, child range - equals OracleEnv.search_tree, read_root_visits agrees, the four slots of
    a board hold the same arrays.  HashNet runs on the device; the peaked and the uniform evaluator go through
    xq_engine_read_leaves / xq_engine_write_priors (moves[64..], priors[64..]).  Widths are asserted on the device's side."""
    from chinesechessai_amd.engine import SelfPlayEngine
    envs, boards, st = _roots(wp.ALL_NAMES, REP)
    eng = SelfPlayEngine(len(envs), sims=sims)
    ev = _engine_evaluator(evaluator)
    ev.bind(eng)
    eng.set_roots(boards, st)
    eng.search(ev)
    moves, visits, n = eng.root_visits()
    nodes = 0
    for b, name in enumerate(wp.ALL_NAMES):
        ref = wp.oracle_tree(name, sims, evaluator)
        f, k = int(ref["first_child"][0]), int(ref["n_child"][0])
        for r in range(REP):
            g = REP * b + r
            t = eng.read_tree(g)
            if r == 0:
                t0 = t
                _equals_oracle_tree(t, ref, (name, sims, evaluator))
                assert int(t["n_child"][0]) == wp.entry(name)[1] >= 64
                nodes += len(t["move"])
            else:
                _same_as_slot(t, t0, (name, sims, evaluator, r))
            assert int(n[g]) == k and moves[g, :k].tolist() == ref["move"][f:f + k].tolist(), (name, g)
            assert visits[g, :k].tolist() == ref["visit_count"][f:f + k].tolist(), (name, g)
            assert (moves[g, k:] == 0).all() and (visits[g, k:] == 0).all(), (name, g)
    eng.close()
    print("wide roots, %s, S = %d: %d nodes equal the oracle's" % (evaluator, sims, nodes))


# ---- b: the generic kernel (virtual loss) against the mirror -----------------------------------------------------------
@pytest.mark.parametrize("sims", [24, 200])
def test_generic_kernel_with_virtual_loss_equals_the_mirror_at_wide_roots(L, sims):
    """search_round_generic + consume_eval<VL> + select_child<VL> at wide nodes: eight pending leaves per game and round,
    the peaked evaluator by planes; every tree equals search_mirror(virtual_loss=True) node by node in child order, no
    pending visit is left, the four slots of a board agree.  Every board, `w128` with its 128-child root (lane 63 carries
    child 127) included: tests/test_wide_nodes_cpu.py walks these mirror trees against the 128-candidate cap."""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import SelfPlayEngine
    envs, boards, st = _roots(wp.ALL_NAMES, REP)
    eng = SelfPlayEngine(len(envs), sims=sims, planes_format=_lib.PLANES_NCHW_F32)
    eng.set_virtual_loss(True)
    ev = PlanesPeakedEvaluator()
    ev.bind(eng)
    eng.set_roots(boards, st)
    eng.search(ev)
    widest = 0
    for b, name in enumerate(wp.ALL_NAMES):
        exp = sm.flatten_nodes(wp.vl_mirror(name, sims))
        for r in range(REP):
            t = eng.read_tree(REP * b + r)
            if r == 0:
                t0 = t
                got = sm.flatten_arrays(t, t["root"])
                assert t["root"] == 0 and len(got) == len(exp), (name, sims, len(got), len(exp))
                for k, (x, y) in enumerate(zip(got, exp)):
                    assert x == y, (name, sims, k, x, y)
                assert int(t["n_child"][0]) == wp.entry(name)[1]
                widest = max(widest, int(t["n_child"][1:].max()))
            else:
                _same_as_slot(t, t0, (name, sims, r))
    assert (eng.tree_stats()[1] == 0).all()
    eng.close()
    assert widest > 64, widest                                    # a wide node below the root was expanded on the device
    print("virtual loss at wide roots, S = %d: widest node below a root %d" % (sims, widest))


# ---- c: tree reuse -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("virtual_loss", [False, True])
def test_reused_trees_from_both_sides_wide_boards_equal_the_mirror(L, virtual_loss):
    """3 plies of argmax play at S = 64 with tree reuse from the boards where both sides are wide: every ply's root - the
    played child's kept subtree from ply 1 on - has more than 64 children; each ply's tree equals play_reuse_mirror's node
    by node (move, N, W bits, P bits, child count, first child), then the played moves and stored visit counts."""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import CallbackEvaluator, SelfPlayEngine
    S, PLIES = 64, 3
    names = wp.BOTH_WIDE
    ref = [sm.play_reuse_mirror(S, PLIES, virtual_loss=virtual_loss, start_env=wp.env_of(n)) for n in names]
    envs, boards, st = _roots(names, REP)
    eng = SelfPlayEngine(len(envs), sims=S, temperature=0.0, max_moves=8,
                         planes_format=_lib.PLANES_NCHW_F32 if virtual_loss else _lib.PLANES_NONE)
    eng.set_tree_reuse(True)
    if virtual_loss:
        eng.set_virtual_loss(True)
        ev = PlanesPeakedEvaluator()
    else:
        ev = CallbackEvaluator(sm.PeakedNet())
    ev.bind(eng)
    eng.set_roots(boards, st)
    kept = 0
    for ply in range(PLIES):
        eng.search(ev)
        for b, name in enumerate(names):
            exp = ref[b][ply]
            for r in range(REP):
                t = eng.read_tree(REP * b + r)
                if r > 0:
                    _same_as_slot(t, t0, (name, ply, r))
                    continue
                t0 = t
                assert t["root"] == exp["root_idx"], (name, ply, t["root"], exp["root_idx"])
                got = sm.flatten_arrays(t, t["root"])
                assert len(got) == len(exp["flat"]), (name, ply, len(got), len(exp["flat"]))
                for k, (x, y) in enumerate(zip(got, exp["flat"])):
                    assert x == y, (name, ply, k, x, y)
                assert int(t["n_child"][t["root"]]) > 64, (name, ply)
                kept += t["root"] != 0
        _lib.check(eng.L.xq_engine_play_move(eng.h))
    _lib.check(eng.L.xq_engine_finalize(eng.h))
    bt = eng.read_results()
    if virtual_loss:
        assert (eng.tree_stats()[1] == 0).all()
    eng.close()
    assert kept >= len(names), kept                                # kept subtrees with wide roots were searched
    assert (bt.n_plies == PLIES).all() and int(bt.error.sum()) == 0
    for b, name in enumerate(names):
        for ply in range(PLIES):
            exp = ref[b][ply]
            n = len(exp["moves"])
            for g in range(REP * b, REP * b + REP):
                assert int(bt.chosen[g, ply]) == exp["played"] and int(bt.s_n[g, ply]) == n, (name, ply, g)
                assert bt.s_moves[g, ply, :n].tolist() == exp["moves"], (name, ply, g)
                assert bt.s_counts[g, ply, :n].tolist() == exp["counts"], (name, ply, g)


# ---- d: plies through the sampler --------------------------------------------------------------------------------------
SAMPLER_SIMS, SAMPLER_PLIES = 50, 3
PICKS = ("63", "64", "last", "below_step", "at_step")


def _probabilities(counts, T):
    """self_play.py:224-231 with NumPy, the sum as np.add.reduce forms it (xqo_np_sum)"""
    from oracle import xq_oracle as xo
    counts = np.asarray(counts, dtype=np.int64)
    if T < 0.01:
        p = np.zeros(len(counts))
        p[np.argmax(counts)] = 1
        return p
    c = np.ascontiguousarray(counts ** (1.0 / T), dtype=np.float64)
    return c / xo.lib().xqo_np_sum(c.ctypes.data_as(C.POINTER(C.c_double)), len(c))


def _uniform_for(p, pick):
    """the double np.random.choice would have to draw for the pick to land where `pick` says, from the reference cdf
    (cumsum / last): inside the step of child 63 / 64 / the last child - or of the nearest visited child below, where that
    one has no visits or does not exist -, and one ulp below / exactly on the upper end of the step of the first visited
    child of the upper half (the lower half's last where there is none): RandomState.choice searches with side='right',
    so the value on the step belongs to the next visited child"""
    cdf = np.cumsum(p)
    cdf = cdf / cdf[-1]
    n = len(p)
    nz = np.nonzero(p)[0]

    def at_or_below(j):
        below = nz[nz <= min(j, n - 1)]
        return int(below[-1]) if len(below) else int(nz[0])
    if pick in ("63", "64", "last"):
        j = at_or_below({"63": 63, "64": 64, "last": n - 1}[pick])
        lo = cdf[j - 1] if j > 0 else 0.0
        return 0.5 * (lo + cdf[j])
    upper = nz[nz >= 64]
    j = int(upper[0]) if len(upper) else int(nz[-1])
    if j == int(nz[-1]):                                      # the last step ends at 1.0, which is never drawn: use the one before
        if len(nz) == 1:
            return float(np.nextafter(cdf[j], 0.0))
        j = int(nz[-2])
    return float(np.nextafter(cdf[j], 0.0)) if pick == "below_step" else float(cdf[j])


def sampler_plan(T, names=None, oracle_evaluator=None, sims=SAMPLER_SIMS, n_plies=SAMPLER_PLIES):
    """The reference side of the sampler test, on the CPU alone: per (board, pick rule) three plies from the board with the
    edge evaluator at S = 50 - the oracle's root visits, pi, the uniform chosen from the reference cdf, the index
    xqo_choice_from_uniform picks, the move, its reward and the game's end.  Every searched tree stays within the
    128-candidate contract (asserted)."""
    from oracle import xq_oracle as xo
    lib = xo.lib()
    ev = oracle_evaluator or wp.edge_oracle_evaluator()
    games = []
    for name in names or wp.SAMPLER_NAMES:
        for pick in PICKS:
            oe = wp.env_of(name)
            plies = []
            for ply in range(n_plies):
                tree = oe.search_tree(sims, ev)
                assert wp.max_candidates(oe, tree) <= wp.MAX_CANDIDATES, (name, pick, ply)
                f, n = int(tree["first_child"][0]), int(tree["n_child"][0])
                moves, counts = tree["move"][f:f + n].tolist(), tree["visit_count"][f:f + n].tolist()
                p = _probabilities(counts, T)
                u = _uniform_for(p, pick)
                idx = lib.xqo_choice_from_uniform(p.ctypes.data_as(C.POINTER(C.c_double)), n, u)
                assert 0 <= idx < n and counts[idx] > 0, (name, pick, ply, idx)
                side = int(oe.e.current_player)
                board = oe.board().reshape(90)
                reward, done, _ = oe.make_move(moves[idx])
                plies.append(dict(moves=moves, counts=counts, p=p, u=u, idx=idx, move=moves[idx], side=side, board=board,
                                  reward=reward))
                if done:
                    break
            w = int(oe.e.winner)
            games.append(dict(name=name, pick=pick, plies=plies, winner=0 if w == xo.WINNER_NONE else w))
    return games


@pytest.mark.parametrize("T", [1.0, 0.5, 0.001])
def test_plies_through_the_sampler_at_wide_roots(L, T):
    """k_play_move's s_moves / s_counts stores, its cdf and binary search over up to 128 entries (T = 1, the pow table of
    T = 0.5, the argmax of T < 0.01), pack_samples and the replay ring on records with more than 64 moves.  Per board
    five games whose uniforms are chosen from the reference cdf (`_uniform_for`): at T >= 0.01 the first ply of every
    board wider than 64 picks child 63, child 64 and the last child exactly, and both sides of a cdf step of the upper
    half.  chosen, s_n, s_moves, s_counts (all 128 entries), game_data's pi bits and z equal the CPU plan; the packed
    records equal read_samples and come back unchanged through a replay ring smaller than the push."""
    from chinesechessai_amd.engine import CallbackEvaluator
    plan = sampler_plan(T)
    if T >= 0.01:                                             # the picks land where they are meant to (ply 0, wide boards)
        for gm in plan:
            n = len(gm["plies"][0]["moves"])
            if n > 64:
                idx = gm["plies"][0]["idx"]
                step = 64 if n > 65 else 63                   # (n = 65: child 64 is the last one, the step before it is 63's)
                assert {"63": idx == 63, "64": idx == 64, "last": idx == n - 1, "below_step": idx == step,
                        "at_step": idx > step}[gm["pick"]], (gm["name"], gm["pick"], idx, n)
    wide = _play_the_plan(T, plan, CallbackEvaluator(wp.EdgeNet()), SAMPLER_SIMS, SAMPLER_PLIES)
    assert wide >= len(wp.SAMPLER_NAMES) * len(PICKS) - len(PICKS)            # (w64's records hold exactly 64 moves)
    print("sampler at T = %g: %d games x %d plies, %d records wider than 64 moves" % (T, len(plan), SAMPLER_PLIES, wide))


@pytest.mark.parametrize("T", [1.0, 0.5])
def test_one_ply_through_the_sampler_at_128_children(L, T):
    """The same at the cap: board `w128`, one ply with HashNet at S = 200 (the tree whose every expanded node
    tests/test_wide_nodes_cpu.py holds against the 128-candidate contract): 128 moves and counts stored, the cdf and the
    binary search over 128 entries with visited children in the upper half, the record through pack_samples and replay."""
    from chinesechessai_amd.engine import HashNetEvaluator
    from oracle import xq_oracle as xo
    plan = sampler_plan(T, wp.SAMPLER_ONE_PLY, xo.hashnet_evaluator(), 200, 1)
    for gm in plan:
        pl = gm["plies"][0]
        assert len(pl["moves"]) == 128 and sum(c > 0 for c in pl["counts"][64:]) >= 3
        assert pl["idx"] >= (64 if gm["pick"] in ("last", "below_step", "at_step") else 0), (gm["pick"], pl["idx"])
    assert len({gm["plies"][0]["idx"] for gm in plan}) >= 4
    wide = _play_the_plan(T, plan, HashNetEvaluator(), 200, 1)
    assert wide == len(plan)


def _play_the_plan(T, plan, ev, sims, n_plies):
    """the engine's side of a sampler plan and every comparison with it; returns the number of records wider than 64"""
    import torch
    from chinesechessai_amd import _lib, distributed as xd
    from chinesechessai_amd.engine import SelfPlayEngine
    from chinesechessai_amd.chess_env import decode_move
    from chinesechessai_amd.replay import ReplayBuffer, pack_board_words
    from oracle import xq_oracle as xo
    G = len(plan)
    envs, boards, st = _roots([gm["name"] for gm in plan])
    eng = SelfPlayEngine(G, sims=sims, temperature=T, max_moves=n_plies)
    ev.bind(eng)
    eng.set_roots(boards, st)
    u = np.zeros((G, _lib.MAX_PLIES))
    for g, gm in enumerate(plan):
        u[g, :len(gm["plies"])] = [p["u"] for p in gm["plies"]]
    eng.set_uniforms(u)
    for _ in range(n_plies):
        eng.search(ev)
        _lib.check(eng.L.xq_engine_play_move(eng.h))
    _lib.check(eng.L.xq_engine_finalize(eng.h))
    bt = eng.read_results()
    rec_t = torch.zeros(G * _lib.MAX_PLIES * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    eng.pack_samples(rec_t.data_ptr())
    torch.cuda.synchronize()
    eng.close()
    rec = xd.records_to_numpy(rec_t).reshape(G, _lib.MAX_PLIES)
    assert int(bt.error.sum()) == 0
    wide_records = 0
    for g, gm in enumerate(plan):
        ctx = (gm["name"], gm["pick"], T)
        k = len(gm["plies"])
        assert int(bt.n_plies[g]) == int(bt.n_samples[g]) == k and int(bt.winner[g]) == gm["winner"], ctx
        data = bt.game_data(g)
        for i, pl in enumerate(gm["plies"]):
            n = len(pl["moves"])
            full_m, full_c = np.zeros(128, np.uint16), np.zeros(128, np.uint16)
            full_m[:n], full_c[:n] = pl["moves"], pl["counts"]
            assert int(bt.chosen[g, i]) == pl["move"] and int(bt.s_n[g, i]) == n, (ctx, i)
            assert np.array_equal(bt.s_moves[g, i], full_m) and np.array_equal(bt.s_counts[g, i], full_c), (ctx, i)
            assert int(bt.s_player[g, i]) == pl["side"] and np.array_equal(bt.s_board[g, i], pl["board"]), (ctx, i)
            pi = np.array([data[i][1][decode_move(m)] for m in pl["moves"]], dtype=np.float64)
            assert pi.tobytes() == pl["p"].tobytes(), (ctx, i)
            z = xo.lib().xqo_z_value(gm["winner"], pl["side"], k, 1, pl["reward"])
            assert struct.pack("<d", z) == struct.pack("<d", float(bt.s_z[g, i])), (ctx, i)
            # the packed record of the sample
            r = rec[g, i]
            assert int(r["valid"]) == 1 and int(r["n_moves"]) == n and int(r["chosen"]) == pl["move"], (ctx, i)
            assert int(r["player"]) == pl["side"] and np.array_equal(r["board"], pack_board_words(pl["board"])), (ctx, i)
            assert np.array_equal(r["moves"], bt.s_moves[g, i]) and np.array_equal(r["counts"], bt.s_counts[g, i]), (ctx, i)
            assert r["z"].tobytes() == bt.s_z[g, i].tobytes(), (ctx, i)
            wide_records += n > 64
        assert not rec[g, k:]["valid"].any(), ctx
    # a push larger than the ring: the ring keeps the newest records, in game / ply order, unchanged
    valid = rec.reshape(-1)[rec.reshape(-1)["valid"] != 0]
    cap = len(valid) // 2 + 1
    rb = ReplayBuffer(max_size=cap)
    assert rb.push_records(rec_t, G) == len(valid) and len(rb) == cap
    back = np.zeros(cap, dtype=xd.RECORD_DTYPE)
    idx = np.arange(cap, dtype=np.int64)
    rb._chk(rb.L.xq_replay_read_records(rb.h, C.c_void_p(rb._stream()), _lib.ptr(idx), cap, _lib.ptr(back)))
    rb.close()
    assert back.tobytes() == valid[-cap:].tobytes()
    assert int((back["n_moves"] > 64).sum()) > 0
    return wide_records


# ---- e: logit gather and softmax against float64 -----------------------------------------------------------------------
ROW_KINDS = ("normal", "equal", "spread", "max63", "max64", "maxlast")


def _legal_logits(rng, kind, n):
    if kind == "normal":
        return rng.normal(0.0, 5.0, n)
    if kind == "equal":
        return np.full(n, 1.25)
    if kind == "spread":
        x = np.where(np.arange(n) % 2 == 0, 80.0, -80.0)
        x[min(64, n - 1)] = 80.0
        return x
    x = rng.normal(0.0, 5.0, n)
    x[{"max63": min(63, n - 1), "max64": min(64, n - 1), "maxlast": n - 1}[kind]] = 30.0
    return x


def _softmax32(x):
    """neural_network.py:148-169 as NumPy evaluates it in float32"""
    x = np.asarray(x, dtype=np.float32)
    e = np.exp(x - x.max())
    return e / e.sum()


def _softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


def _rel_err(p, p64):
    """largest |p - p64| / p64 over the entries float32 holds as normal numbers"""
    ok = p64 >= 2.0 ** -126
    return float(np.max(np.abs(p[ok].astype(np.float64) - p64[ok]) / p64[ok]))


@pytest.mark.parametrize("consumer", ["round", "end_search", "virtual_loss"])
@pytest.mark.parametrize("compaction", [False, True])
@pytest.mark.parametrize("layout", ["all", "reachable"])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_logit_gather_and_softmax_at_wide_roots(L, kind, layout, compaction, consumer):
    """The x1 / e1 / p1 half of the logit gather and its store of children 64.., with no network: after round 0 every
    root waits for its evaluation; seeded synthetic logits (float32 or bf16; 8,100 columns or the 2,304 compact ones behind
    xq_engine_set_logit_columns; by slot or by compacted row with the row map fetched) are consumed by each of the three
    places that gather logits - round 1 of the one-leaf kernel, xq_engine_end_search (consume_eval<false>; sims = 8, one
    round) and round 1 of the generic kernel under virtual loss (consume_eval<true>, eight rows per game) - and
    read_root_priors is compared with a softmax over the legal columns: float32 on the host (rtol 2e-6, atol 1e-9, the
    suite's bound), float64 (the device may err twice as much as NumPy's float32 softmax does: expf and a 128-term
    butterfly sum cost a few ulps each; both figures are printed).  Rows: N(0, 5^2); all equal (the priors are the bits of
    float32(1) / float32(n)); +-80 (priors underflow to exactly 0, the others still sum to 1); the maximum on child 63,
    child 64, the last child.  Every other column holds noise the gather must not read; entries from n on are 0."""
    import torch
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import SelfPlayEngine
    from chinesechessai_amd.neural_network import reachable_policy_columns
    names = [n for n in wp.ALL_NAMES for _ in ROW_KINDS]
    G = len(names)
    envs, boards, st = _roots(names)
    if layout == "reachable":
        cols, cmap = reachable_policy_columns()
        stride = (len(cols) + 191) // 192 * 192
    else:
        cmap, stride = None, 8100
    eng = SelfPlayEngine(G, sims=8 if consumer == "end_search" else 16)
    if consumer == "virtual_loss":
        eng.set_virtual_loss(True)
    K = eng.n_rows // G                                       # evaluator rows per game: 1, or 8 under virtual loss
    assert K == (8 if consumer == "virtual_loss" else 1)
    _lib.check(eng.L.xq_engine_set_logit_columns(eng.h, _lib.ptr(cmap) if cmap is not None else None,
                                                 stride if cmap is not None else 0))
    eng.set_row_compaction(compaction)
    if compaction:
        assert all(eng.row_map())
    eng.set_roots(boards, st)
    _lib.check(eng.L.xq_engine_search_round(eng.h, 0, _lib.EVAL_PRIORS, None, None, None))
    if compaction:                                            # the row of the game's one pending leaf (the root)
        lr = eng.leaf_rows().reshape(G, K)
        assert ((lr >= 0).sum(axis=1) == 1).all() and sorted(lr[lr >= 0].tolist()) == list(range(G))
        rows = [[int(r) for r in lr[g] if r >= 0] for g in range(G)]
    else:                                                     # by slot: whichever of the game's slots holds the leaf
        rows = [list(range(K * g, K * g + K)) for g in range(G)]
    rng = np.random.RandomState(20261021)
    host = rng.normal(0.0, 5.0, (G * K, stride)).astype(np.float32)
    legal = []
    for g, name in enumerate(names):
        mv = np.asarray(envs[g].legal_moves(), dtype=np.int64)
        x = _legal_logits(rng, ROW_KINDS[g % len(ROW_KINDS)], len(mv)).astype(np.float32)
        for r in rows[g]:
            host[r, cmap[mv].astype(np.int64) if cmap is not None else mv] = x
        legal.append(mv)
    rows = [r[0] for r in rows]
    dev = torch.from_numpy(host).cuda()
    if kind == "bf16":
        dev = dev.bfloat16()
        host = dev.float().cpu().numpy()                      # what the device reads
    vals = torch.zeros(G * K, device="cuda", dtype=dev.dtype)
    code = _lib.EVAL_LOGITS_BF16 if kind == "bf16" else _lib.EVAL_LOGITS_F32
    if consumer == "end_search":
        assert eng.rounds == 1
        _lib.check(eng.L.xq_engine_end_search(eng.h, code, C.c_void_p(dev.data_ptr()), C.c_void_p(vals.data_ptr())))
    else:
        _lib.check(eng.L.xq_engine_search_round(eng.h, 1, code, C.c_void_p(dev.data_ptr()), C.c_void_p(vals.data_ptr()), None))
    pri = eng.root_priors()
    eng.close()
    err_dev = err_np = 0.0
    for g, name in enumerate(names):
        mv, n, rk = legal[g], len(legal[g]), ROW_KINDS[g % len(ROW_KINDS)]
        x = host[rows[g], cmap[mv].astype(np.int64) if cmap is not None else mv]
        p32, p64 = _softmax32(x), _softmax64(x)
        got = pri[g, :n]
        assert n == wp.entry(name)[1] and (pri[g, n:] == 0).all(), (name, rk)
        assert np.allclose(got, p32, rtol=2e-6, atol=1e-9), (name, rk, float(np.abs(got - p32).max()))
        assert abs(float(got.astype(np.float64).sum()) - 1.0) < 1e-5, (name, rk)
        if rk == "equal":
            assert (got.view(np.uint32) == (np.float32(1) / np.float32(n)).view(np.uint32)).all(), (name, n)
        if rk == "spread":
            low = x < 0
            assert low.any() and (got[low] == 0).all() and (got[~low] > 0).all(), name
        if rk in ("max63", "max64", "maxlast"):
            assert int(np.argmax(got)) == {"max63": min(63, n - 1), "max64": min(64, n - 1), "maxlast": n - 1}[rk], (name, rk)
        err_dev, err_np = max(err_dev, _rel_err(got, p64)), max(err_np, _rel_err(p32, p64))
    print("softmax over up to 128 legal logits (%s, %s columns, %s, consumed by %s): largest relative error against float64: "
          "device %.3g, NumPy float32 %.3g" % (kind, layout, "compacted rows" if compaction else "rows by slot", consumer,
                                               err_dev, err_np))
    assert err_dev <= 2 * err_np, (err_dev, err_np)


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_network_logits_reach_wide_roots_as_their_softmax(L, dtype):
    """The same through TorchNetEvaluator - the hand-written bf16 path (compact columns, compacted rows) and the fp32
    parity path - on a seeded 1-block ChessNet whose policy_fc weight and bias are multiplied by 40 before folding (a
    peaked policy): the logits the network wrote for round 0 are read back, round 1 consumes those very logits, and the
    root priors equal the host's float32 softmax of them over the legal columns (rtol 2e-6, atol 1e-9)."""
    import torch
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    torch.manual_seed(20261021)
    net = ChessNet(num_blocks=1).eval()
    with torch.no_grad():
        net.policy_fc.weight.mul_(40.0)
        net.policy_fc.bias.mul_(40.0)
    net = net.cuda()
    bf = dtype == "bfloat16"
    ev = TorchNetEvaluator(net, dtype=torch.bfloat16 if bf else torch.float32, channels_last=bf, eval_cache=False)
    envs, boards, st = _roots(wp.ALL_NAMES)
    G = len(envs)
    eng = SelfPlayEngine(G, sims=16, planes_format=ev.planes_format)
    eng.set_root_eval_carry(False)
    eng._bind(ev)
    assert eng.row_compaction == bf
    eng.set_roots(boards, st)
    _lib.check(eng.L.xq_engine_search_round(eng.h, 0, _lib.EVAL_PRIORS, None, None, ev.planes_ptr()))
    code, a, v = ev.evaluate(eng)
    torch.cuda.synchronize()
    rows = eng.leaf_rows()
    assert (rows >= 0).all()
    logits = ev.logits.float().cpu().numpy()[rows]
    _lib.check(eng.L.xq_engine_search_round(eng.h, 1, code, C.c_void_p(a), C.c_void_p(v), ev.planes_ptr()))
    pri = eng.root_priors()
    eng.close()
    cmap = ev.inet.column_map
    peak = 0.0
    for g, name in enumerate(wp.ALL_NAMES):
        mv = np.asarray(envs[g].legal_moves(), dtype=np.int64)
        n = len(mv)
        x = logits[g, cmap[mv].astype(np.int64) if cmap is not None else mv]
        p32 = _softmax32(x)
        assert np.allclose(pri[g, :n], p32, rtol=2e-6, atol=1e-9), (name, dtype, float(np.abs(pri[g, :n] - p32).max()))
        assert (pri[g, n:] == 0).all() and abs(float(pri[g, :n].astype(np.float64).sum()) - 1.0) < 1e-5, (name, dtype)
        peak = max(peak, float(x.max() - x.min()))
    print("network logits at wide roots (%s): widest logit range %.1f" % (dtype, peak))


# ---- f: work elimination at wide nodes ---------------------------------------------------------------------------------
def test_work_elimination_is_result_identical_at_wide_nodes(L):
    """Leaf dedupe, root evaluation carry-over and the evaluation cache (eval_cache_fill and the verify compare at n > 64,
    the j1 half of k_play_move's carry-over) against the plain path: the three both-sides-wide boards in 64 slots each
    with distinct uniform streams, 4 plies, a seeded bf16 network, S = 48.  Records and outcomes are identical with all
    three on and with all three off; the cache answers; verify mode compares and finds no mismatch; and at some ply >= 1
    more roots are wider than 64 than roots_not_ready reported as needing a fresh evaluation: a carried root was wide."""
    import torch
    from chinesechessai_amd import _lib, distributed as xd
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    S, PLIES, REPS = 48, 4, 64
    torch.manual_seed(20261022)
    net = ChessNet(num_blocks=1).eval().cuda()
    envs, boards, st = _roots(wp.BOTH_WIDE, REPS)
    G = len(envs)
    u = np.zeros((G, _lib.MAX_PLIES))
    for g in range(G):
        u[g, :PLIES] = np.random.RandomState(1000 + g).random_sample(PLIES)
    inet = []

    def run(on, cache):
        ev = TorchNetEvaluator(inet[0] if inet else net, leaf_dedupe=on, eval_cache=cache)
        if not inet:
            inet.append(ev.inet)
        eng = SelfPlayEngine(G, sims=S, planes_format=ev.planes_format, max_moves=PLIES)
        eng.set_root_eval_carry(on)
        eng._bind(ev)
        assert eng.leaf_dedupe == on and eng.eval_cache == bool(cache) and eng.row_compaction
        eng.set_roots(boards, st)
        eng.set_uniforms(u)
        not_ready = []
        for _ in range(PLIES):
            eng.search(ev)
            _lib.check(eng.L.xq_engine_play_move(eng.h))
            not_ready.append(eng.roots_not_ready())
        _lib.check(eng.L.xq_engine_finalize(eng.h))
        t = torch.zeros(G * _lib.MAX_PLIES * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
        eng.pack_samples(t.data_ptr())
        out = eng.read_game_outcomes()
        stats = eng.eval_cache_stats() if cache else (0, 0, 0)
        eng.close()
        return xd.records_to_numpy(t).reshape(G, _lib.MAX_PLIES), out, stats, not_ready

    ref, ref_out, _, _ = run(False, False)
    assert int(ref_out["error"].sum()) == 0
    assert (ref[:, 0]["n_moves"] > 64).all()
    rec, out, (hits, fills, _), not_ready = run(True, "on")
    rec_v, out_v, (compared, _, bad), _ = run(True, "verify")
    for k in ("winner", "reason", "reason_side", "reason_count", "n_plies", "n_samples", "error"):
        assert np.array_equal(out[k], ref_out[k]) and np.array_equal(out_v[k], ref_out[k]), k
    for g in range(G):
        _same_game(rec[g], ref[g], ("on", g))
        _same_game(rec_v[g], ref[g], ("verify", g))
    assert hits > 0 and fills > 0, (hits, fills)
    assert compared > 0 and bad == 0, (compared, bad)
    wide = [int((rec[:, ply]["n_moves"] > 64).sum()) for ply in range(PLIES)]
    # pigeonhole: not_ready[ply - 1] roots were NOT carried into `ply`; more roots than that are wider than 64 there, so at
    # least one of the wide roots was carried
    assert any(not_ready[ply - 1] < G and wide[ply] > not_ready[ply - 1] for ply in range(1, PLIES)), (wide, not_ready)
    print("work elimination at wide nodes: roots wider than 64 per ply %s, roots not carried per ply %s, cache hits %d, "
          "fills %d, verify compared %d" % (wide, not_ready, hits, fills, compared))


# ---- g: root noise -----------------------------------------------------------------------------------------------------
def test_root_noise_is_a_dirichlet_sample_on_both_halves_of_a_wide_root(L):
    """root_noise's g1 half: board `w104` (n = 104, the widest board below 128) in all 16,384 slots at sims = 16 with
    alpha = 0.3, eps = 0.25.  eta = (P' - (1 - eps) P) / eps is non-negative, sums to 1, is deterministic per seed, and over
    the slots every child's mean is 1/n within 0.001 and its variance (1/n)(1 - 1/n)/(n alpha + 1) within a quarter -
    reported for children below and from index 64 on.  NumPy's own dirichlet([0.3] * 104, size=16384) over 20 seeds shows
    at worst |var / theory - 1| = 0.134 and |mean - 1/n| = 0.00051: the bounds (the ones the suite's narrower noise test and
    its issue set) are 1.9 times what an exact sampler shows at this n and slot count."""
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    name = "w104"
    assert wp.entry(name)[1] == max(b[1] for b in wp.BOARDS if b[1] <= 127)
    G, alpha, eps, n = 16384, 0.3, 0.25, 104
    envs, boards, st = _roots([name])
    boards, st = np.repeat(boards, G, axis=0), np.repeat(st, G, axis=0)
    ev = HashNetEvaluator()

    def root_priors(seed):
        eng = SelfPlayEngine(G, sims=16)
        if seed is not None:
            eng.set_root_noise(alpha, eps, seed)
        eng.set_roots(boards, st)
        eng.search(ev)
        p = eng.root_priors()
        eng.close()
        return p

    clean = root_priors(None)
    assert (clean[:, n:] == 0).all() and (clean[:, :n] > 0).all() and (clean == clean[0]).all()
    a, b, c = root_priors(1), root_priors(1), root_priors(2)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert (a[:, n:] == 0).all()
    eta = (a[:, :n].astype(np.float64) - (1 - eps) * clean[:, :n]) / eps
    assert eta.min() > -1e-5 and np.abs(eta.sum(axis=1) - 1).max() < 1e-4
    var = (1.0 / n) * (1 - 1.0 / n) / (n * alpha + 1)
    dm, dv = np.abs(eta.mean(axis=0) - 1.0 / n), np.abs(eta.var(axis=0) / var - 1)
    print("root noise at n = %d over %d slots: worst |mean - 1/n| %.5f (children 0..63) %.5f (64..%d); worst |var/theory - 1| "
          "%.3f (0..63) %.3f (64..%d)" % (n, G, dm[:64].max(), dm[64:].max(), n - 1, dv[:64].max(), dv[64:].max(), n - 1))
    assert dm.max() < 0.001 and dv.max() < 0.25
    assert len({a[g].tobytes() for g in range(64)}) == 64


# ---- h: two networks ---------------------------------------------------------------------------------------------------
def test_two_networks_at_wide_red_and_black_roots(L):
    """One per-slot ply (xq_engine_search_round2 / end_search2, pairing 1, HashNet salts 0 and 1) at every wide board and at
    `heavy_both` with black to move: each tree equals the oracle's with the salt of the side to move at the root - network
    0 for the red roots, network 1 for the black ones."""
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    from oracle import xq_oracle as xo
    S = 50
    roots = [(n, wp.entry(n)[4]) for n in wp.ALL_NAMES] + [("heavy_both", -1)]
    envs = [wp.env_of(n, side) for n, side in roots for _ in range(REP)]
    assert {side for _, side in roots} == {1, -1}
    boards, st = _state_rows(envs)
    ev0, ev1 = HashNetEvaluator(0), HashNetEvaluator(1)
    eng = SelfPlayEngine(len(envs), sims=S)
    eng._bind(ev0, ev1, per_slot=True)
    eng.set_roots(boards, st)
    eng.set_pairing(np.ones(len(envs), np.uint8))
    eng.search(ev0, ev1, per_slot=True)
    black_wide = 0
    for b, (name, side) in enumerate(roots):
        oe = envs[REP * b]
        ref = oe.search_tree(S, None if side == 1 else _salted(1))
        assert wp.max_candidates(oe, ref) <= wp.MAX_CANDIDATES, (name, side)
        for r in range(REP):
            t = eng.read_tree(REP * b + r)
            if r == 0:
                t0 = t
                _equals_oracle_tree(t, ref, (name, side))
                assert int(t["n_child"][0]) > 64 or name == "w64"
                black_wide += side == -1 and int(t["n_child"][0]) > 64
            else:
                _same_as_slot(t, t0, (name, side, r))
    eng.close()
    assert black_wide == 2
    # the salts do differ at these roots: the other network's tree is another tree
    oe = wp.env_of("lawful_both_black")
    assert oe.search_tree(S)["visit_count"].tobytes() != oe.search_tree(S, _salted(1))["visit_count"].tobytes()
