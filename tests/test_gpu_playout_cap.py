"""GPU tests (`-m gpu`) of playout cap randomization (xq_engine_set_playout_cap / SelfPlayEngine.set_playout_cap): each ply
is searched with `sims` simulations (full) or `fast_sims` (fast), decided per game and ply by the switch's seed and the
game's own uniform.  Reference: tests/playout_cap_model.py - one game driven over the CPU oracle's public API, held to
oracle.self_play_game by tests/test_playout_cap_cpu.py.  Every comparison is bit for bit."""
import concurrent.futures as cf

import numpy as np
import pytest

from tests import playout_cap_model as pm

pytestmark = pytest.mark.gpu

S, LB = 50, 8
SEEDS = np.arange(7000, 7064, dtype=np.uint32)
CAP_SEED = 12345
_MODELS = {}


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


def _models(seeds, sims, p, fast, cap_seed=CAP_SEED):
    """model games by seed, computed once per configuration (the oracle's C code runs outside the interpreter lock)"""
    from oracle import xq_oracle as xo
    xo.lib().xqo_crc32(0, None, 0)                                      # (the oracle's one lazily built table, before threads)
    todo = [int(s) for s in seeds if (int(s), sims, p, fast, cap_seed) not in _MODELS]
    if todo:
        with cf.ThreadPoolExecutor(max_workers=8) as ex:
            for s, g in zip(todo, ex.map(lambda s: pm.play(s, sims, p, fast, cap_seed=cap_seed), todo)):
                _MODELS[(s, sims, p, fast, cap_seed)] = g
    return [_MODELS[(int(s), sims, p, fast, cap_seed)] for s in seeds]


def _engine(n, sims=S, **kw):
    from chinesechessai_amd.engine import SelfPlayEngine
    return SelfPlayEngine(n, sims=sims, leaf_batch=LB, **kw)


def _pack(eng, n):
    import torch
    from chinesechessai_amd import distributed as xd
    t = torch.zeros(n * 70 * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    eng.pack_samples(t.data_ptr())
    torch.cuda.synchronize()
    return t, xd.records_to_numpy(t).reshape(n, 70)


def _check_batch_game(b, ps, g, m, ctx):
    """game g of a GameBatch (+ ply_sims) against its model game: moves, counts, pi, z, winner, reason, budgets"""
    assert b.error[g] == 0 and m.error == 0, ctx
    assert (int(b.n_plies[g]), int(b.n_samples[g]), int(b.winner[g]), int(b.reason[g]), int(b.reason_side[g]),
            int(b.reason_count[g])) == (m.n_plies, m.n_samples, m.winner, m.reason, m.reason_side, m.reason_count), ctx
    assert b.chosen[g, :m.n_plies].tolist() == m.chosen, ctx
    data = b.game_data(g)
    for i in range(m.n_samples):
        n = len(m.moves[i])
        assert int(b.s_n[g, i]) == n and b.s_moves[g, i, :n].tolist() == m.moves[i], (ctx, i)
        assert b.s_counts[g, i, :n].tolist() == m.counts[i], (ctx, i)
        assert np.array(list(data[i][1].values()), np.float64).tobytes() == m.pi[i].tobytes(), (ctx, i)
        assert np.float64(b.s_z[g, i]).tobytes() == np.float64(m.z[i]).tobytes(), (ctx, i)
        assert int(b.s_player[g, i]) == m.players[i] and b.s_board[g, i].tobytes() == m.boards[i].tobytes(), (ctx, i)
    assert ps[g, :m.n_samples].tolist() == m.sims and not ps[g, m.n_samples:].any(), ctx


def _check_record_game(rec, m, record_fast, ctx, temperature=1.0):
    """xq_sample_record[70] of one game against its model game; pad / valid against the plan"""
    from chinesechessai_amd.distributed import record_to_sample
    k = m.n_samples
    fast = ~np.array(m.full, bool)
    assert rec["pad"][:k].tolist() == fast.astype(int).tolist() and not rec["pad"][k:].any(), ctx
    want_valid = np.ones(k, bool) if record_fast else ~fast
    assert rec["valid"][:k].tolist() == want_valid.astype(int).tolist() and not rec["valid"][k:].any(), ctx
    for i in range(k):
        n = len(m.moves[i])
        r = rec[i]
        assert int(r["n_moves"]) == n and r["moves"][:n].tolist() == m.moves[i] and r["counts"][:n].tolist() == m.counts[i], (ctx, i)
        assert int(r["chosen"]) == m.chosen[i] and int(r["player"]) == m.players[i], (ctx, i)
        assert r["z"].tobytes() == np.float64(m.z[i]).tobytes(), (ctx, i)
        board, probs, z = record_to_sample(r, temperature)
        assert board.reshape(90).tobytes() == m.boards[i].tobytes(), (ctx, i)
        assert np.array(list(probs.values()), np.float64).tobytes() == m.pi[i].tobytes(), (ctx, i)


# ---- 1. whole games against the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sims,fast", [(50, 9), (50, 16), (50, 20), (50, 49), (20, 12)])
def test_whole_games_equal_the_model(L, sims, fast):
    """64 games, seeds 7000..7063, leaf_batch 8, p = 0.25, lock-step play(): fast budgets whose last round runs 1, 8 and 4
    simulations, one that differs from the full budget in the last round only, and once 20 / 12.  Moves, counts, pi, z,
    winner, reason and ply_sims() equal the model; the packed records' pad / valid bytes equal the plan for both values
    of record_fast."""
    from chinesechessai_amd.engine import HashNetEvaluator
    models = _models(SEEDS, sims, 0.25, fast)
    eng = _engine(len(SEEDS), sims=sims)
    try:
        eng.set_playout_cap(0.25, fast, seed=CAP_SEED)
        b = eng.play(HashNetEvaluator(), SEEDS)
        ps = eng.ply_sims()
        assert np.array_equal(b.ply_sims, ps)
        _, rec = _pack(eng, len(SEEDS))
        eng.set_playout_cap(0.25, fast, seed=CAP_SEED, record_fast=True)
        _, rec_all = _pack(eng, len(SEEDS))
    finally:
        eng.close()
    n_fast = n_full = 0
    for g, m in enumerate(models):
        _check_batch_game(b, ps, g, m, (sims, fast, g))
        _check_record_game(rec[g], m, False, (sims, fast, g))
        _check_record_game(rec_all[g], m, True, (sims, fast, g, "record_fast"))
        n_full += sum(m.full)
        n_fast += m.n_samples - sum(m.full)
    assert n_fast > 0 and n_full > 0


# ---- 2. degenerate forms ------------------------------------------------------------------------------------------------
def test_degenerate_forms_equal_a_run_without_the_switch(L):
    """fast_sims = sims, full_prob = 1, and the switch set and cleared again: every array of read_samples, the outcomes and
    the packed records, byte for byte, equal those of an engine that never touched the switch."""
    from chinesechessai_amd.engine import HashNetEvaluator
    seeds = SEEDS[:24]

    def run(setup):
        eng = _engine(len(seeds))
        try:
            setup(eng)
            b = eng.play(HashNetEvaluator(), seeds)
            ps = eng.ply_sims()
            t, _ = _pack(eng, len(seeds))
            return b, ps, t.cpu().numpy().tobytes()
        finally:
            eng.close()

    def set_and_clear(eng):
        eng.set_playout_cap(0.25, 16, seed=3, record_fast=True)
        eng.set_playout_cap(1.0, 0)

    ref, ref_ps, ref_rec = run(lambda eng: None)
    assert (ref_ps[np.arange(70)[None, :] < ref.n_samples[:, None]] == S).all()
    for name, setup in (("fast_sims = sims", lambda eng: eng.set_playout_cap(0.25, S, seed=3)),
                        ("full_prob = 1", lambda eng: eng.set_playout_cap(1.0, 16, seed=3)),
                        ("set and cleared", set_and_clear)):
        b, ps, rec = run(setup)
        for k in ("winner", "reason", "reason_side", "reason_count", "n_plies", "n_samples", "error", "s_board", "s_player",
                  "s_n", "s_moves", "s_counts", "s_z", "chosen", "step_reward"):
            assert getattr(b, k).tobytes() == getattr(ref, k).tobytes(), (name, k)
        assert np.array_equal(ps, ref_ps), name
        assert rec == ref_rec, name


# ---- 3. rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,fast", [(0.25, 16), (1e-9, 16)])
def test_a_spent_slot_has_no_row(L, p, fast):
    """Row compaction and the root carry-over on, three plies round by round: after every round no slot whose budget is
    spent has a row in leaf_rows() and every slot with budget left has one (round 0: unless its root was carried over;
    nobody meets a terminal leaf three plies from the start position); row_history() of the ply equals the model's count
    per round.  With p tiny every ply is fast and rounds >= ceil(fast_sims / 8) have no row at all."""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import HashNetEvaluator, playout_plan
    G = len(SEEDS)
    u = np.stack([pm.game_uniforms(s) for s in SEEDS])
    full = playout_plan(u, CAP_SEED, p)
    if p < 1e-6:
        assert not full.any()
    eng = _engine(G)
    try:
        ev = HashNetEvaluator()
        ev.bind(eng)
        eng.set_row_compaction(True)
        eng.set_root_eval_carry(True)
        eng.set_playout_cap(p, fast, seed=CAP_SEED)
        eng.new_games(SEEDS)
        R = eng.rounds
        for ply in range(3):
            budget = np.where(full[:, ply], S, fast)
            carried = np.zeros(G, bool) if ply == 0 else np.ones(G, bool)
            if ply:
                assert eng.roots_not_ready() == 0
            eng.row_history(cap=0, reset=True)
            kind, a, v = _lib.EVAL_PRIORS, None, None
            for r in range(R):
                _lib.check(eng.L.xq_engine_search_round(eng.h, r, kind, a, v, None))
                rows = eng.leaf_rows()
                left = budget - r * LB > 0
                want = left & ~carried if r == 0 else left
                assert np.array_equal(rows >= 0, want), (ply, r, np.nonzero((rows >= 0) != want)[0][:8])
                assert sorted(rows[rows >= 0].tolist()) == list(range(int(want.sum()))), (ply, r)
                kind, a, v = ev.evaluate(eng)
            _lib.check(eng.L.xq_engine_end_search(eng.h, kind, a, v))
            hist, n = eng.row_history(cap=R)
            model = [int(((budget - r * LB > 0) & (~carried if r == 0 else True)).sum()) for r in range(R)]
            assert n == R and hist.tolist() == model, (ply, hist.tolist(), model)
            if p < 1e-6:
                assert not hist[-(-fast // LB):].any()
            _, visits, _ = eng.root_visits()
            assert np.array_equal(visits.sum(axis=1), budget - LB), ply      # the first 8 simulations land on the root
            _lib.check(eng.L.xq_engine_play_move(eng.h))
    finally:
        eng.close()


# ---- 4. eliminations ----------------------------------------------------------------------------------------------------
def test_eliminations_equal_the_plain_path(L):
    """A real network, 256 capped games: leaf dedupe, root carry-over and the evaluation cache on give the records of the
    plain path (every root evaluated afresh, one row per pending leaf); in verify mode the cache never disagrees with a
    fresh evaluation."""
    from chinesechessai_amd.engine import TorchNetEvaluator
    from tests.test_gpu_round4 import _mate_line_net
    net = _mate_line_net(2, 11)
    seeds = np.arange(7000, 7256, dtype=np.uint32)

    def run(dedupe, cache, carry):
        ev = TorchNetEvaluator(net, leaf_dedupe=dedupe, eval_cache=cache)
        eng = _engine(len(seeds), planes_format=ev.planes_format)
        try:
            eng.set_root_eval_carry(carry)
            eng.set_playout_cap(0.25, 16, seed=CAP_SEED)
            b = eng.play(ev, seeds)
            facts = dict(carry=eng._carry_on, cache=eng.eval_cache, dedupe=eng.leaf_dedupe, stats=eng.eval_cache_stats(),
                         rows=int(eng.row_history()[0].astype(np.int64).sum()))
            ps = eng.ply_sims()
            t, _ = _pack(eng, len(seeds))
            return b, ps, t.cpu().numpy().tobytes(), facts
        finally:
            eng.close()

    ref, ref_ps, ref_rec, f0 = run(False, False, False)
    assert not f0["carry"] and not f0["cache"] and not f0["dedupe"] and int(ref.error.sum()) == 0
    assert (ref_ps == 16).any() and (ref_ps == S).any()
    for cache in ("on", "verify"):
        b, ps, rec, f = run(True, cache, True)
        assert f["carry"] and f["cache"] and f["dedupe"]
        print("cache %s: hits %d fills %d mismatches %d, rows %d (plain path %d)" % ((cache,) + f["stats"] + (f["rows"], f0["rows"])))
        for k in ("winner", "reason", "reason_side", "reason_count", "n_plies", "n_samples", "error", "s_board", "s_player",
                  "s_n", "s_moves", "s_counts", "s_z", "chosen", "step_reward"):
            assert getattr(b, k).tobytes() == getattr(ref, k).tobytes(), (cache, k)
        assert np.array_equal(ps, ref_ps) and rec == ref_rec, cache
        assert f["rows"] < f0["rows"]
        if cache == "verify":
            assert f["stats"][2] == 0 and f["stats"][0] > 0, f["stats"]


# ---- 5. refill ----------------------------------------------------------------------------------------------------------
def test_refill_games_equal_their_model_games_by_id(L):
    """192 games through 64 slots: every game is its model game, whatever slot and step it started at - k_refill plans a
    restarted slot's first ply from the NEW game's uniform."""
    import torch
    from chinesechessai_amd import distributed as xd
    from chinesechessai_amd.engine import HashNetEvaluator
    seeds = np.arange(7000, 7192, dtype=np.uint32)
    T = len(seeds)
    models = _models(seeds, S, 0.25, 16)
    eng = _engine(64)
    try:
        eng.set_playout_cap(0.25, 16, seed=CAP_SEED)
        rec_t = torch.zeros(T * 70 * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
        out, plies = eng.play_refill(HashNetEvaluator(), seeds, rec_t.data_ptr())
        torch.cuda.synchronize()
        rec = xd.records_to_numpy(rec_t).reshape(T, 70)
    finally:
        eng.close()
    assert int(out["error"].sum()) == 0
    firsts = set()
    for g, m in enumerate(models):
        assert (int(out["n_plies"][g]), int(out["n_samples"][g]), int(out["winner"][g]), int(out["reason"][g]),
                int(out["reason_side"][g]), int(out["reason_count"][g])) == (
            m.n_plies, m.n_samples, m.winner, m.reason, m.reason_side, m.reason_count), g
        _check_record_game(rec[g], m, False, ("refill", g))
        if g >= 64:
            firsts.add(m.full[0])
    assert firsts == {True, False}                                          # restarted slots began with both kinds of ply


# ---- 6. set_roots -------------------------------------------------------------------------------------------------------
def test_set_roots_plans_the_first_ply(L, golden_dir):
    """Twelve positions of tests/golden/rules_random.npz as caller-provided roots: the first ply's budgets equal the plan
    (ply 0 of each slot's uniforms) and the root visits equal OracleEnv.search(budget)."""
    import os
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import HashNetEvaluator, playout_plan
    from oracle import xq_oracle as xo
    d = np.load(os.path.join(golden_dir, "rules_random.npz"))
    idx = np.nonzero((d["winner"] == xo.WINNER_NONE) & (d["nlegal"] > 0) & (d["done"] == 0))[0][5::250][:12]
    assert len(idx) == 12
    seeds = SEEDS[:12]
    u = np.stack([pm.game_uniforms(s) for s in seeds])
    budget = np.where(playout_plan(u[:, 0], 1, 0.5), S, 20)
    assert 0 < (budget == S).sum() < 12
    st = np.zeros((12, _lib.STATE_WORDS), np.int32)
    st[:, _lib.S_PLAYER], st[:, _lib.S_MOVE_COUNT], st[:, _lib.S_WINNER] = d["player"][idx], d["move_count"][idx], _lib.WINNER_NONE
    st[:, _lib.S_RED_KING], st[:, _lib.S_BLACK_KING], st[:, _lib.S_NO_CAPTURE] = d["red_king"][idx], d["black_king"][idx], d["no_capture"][idx]
    eng = _engine(12)
    try:
        ev = HashNetEvaluator()
        ev.bind(eng)
        eng.new_games(seeds)
        eng.set_playout_cap(0.5, 20, seed=1)
        eng.set_roots(d["board"][idx], st)
        eng.search(ev)
        moves, visits, n = eng.root_visits()
        _lib.check(eng.L.xq_engine_play_move(eng.h))
        ps = eng.ply_sims()
    finally:
        eng.close()
    assert ps[:, 0].tolist() == budget.tolist() and not ps[:, 1:].any()
    for i, k in enumerate(idx):
        oe = xo.OracleEnv()
        oe.set_state(d["board"][k], d["player"][k], d["move_count"][k], xo.WINNER_NONE, d["red_king"][k], d["black_king"][k],
                     d["no_capture"][k])
        mv, vs = oe.search(int(budget[i]))
        assert moves[i, :n[i]].tolist() == mv and visits[i, :n[i]].tolist() == vs, (i, int(budget[i]))


# ---- 7. noise -----------------------------------------------------------------------------------------------------------
def test_root_noise_at_full_plies_only(L):
    """epsilon = 0.25 with the cap on: the root priors of a fast ply are the noise-free run's bits, those of a full ply
    differ.  Plies 0 and 1; at ply 1 only the games whose ply 0 was fast are compared (a noisy ply 0 may have moved
    elsewhere)."""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import HashNetEvaluator, playout_plan
    G = len(SEEDS)
    full = playout_plan(np.stack([pm.game_uniforms(s) for s in SEEDS]), CAP_SEED, 0.25)

    def run(eps):
        eng = _engine(G)
        try:
            ev = HashNetEvaluator()
            ev.bind(eng)
            eng.set_root_noise(0.3, eps, seed=99)
            eng.set_playout_cap(0.25, 16, seed=CAP_SEED)
            eng.new_games(SEEDS)
            out = []
            for ply in range(2):
                eng.search(ev)
                out.append((eng.root_priors(), eng.root_visits()[2]))
                _lib.check(eng.L.xq_engine_play_move(eng.h))
            return out
        finally:
            eng.close()

    noisy, clean = run(0.25), run(0.0)
    seen = {(0, True): 0, (0, False): 0, (1, True): 0, (1, False): 0}
    for ply in range(2):
        for g in range(G):
            if ply == 1 and full[g, 0]:
                continue
            n = int(clean[ply][1][g])
            assert n == int(noisy[ply][1][g]) and n > 0
            same = noisy[ply][0][g, :n].tobytes() == clean[ply][0][g, :n].tobytes()
            assert same == (not full[g, ply]), (ply, g, bool(full[g, ply]))
            seen[(ply, bool(full[g, ply]))] += 1
    assert all(seen.values()), seen


# ---- 8. replay ----------------------------------------------------------------------------------------------------------
def test_replay_buffer_takes_full_plies_only(L):
    """A capped session's records (record_fast = False) pushed into a ReplayBuffer: its length is the number of full
    plies, xq_replay_read_records returns exactly those plies in game / ply order, and sample_policy_tensors' pi is the
    model's pi (rounded once to float32) for them."""
    import ctypes as C
    from chinesechessai_amd import _lib
    from chinesechessai_amd.distributed import RECORD_DTYPE
    from chinesechessai_amd.engine import HashNetEvaluator
    from chinesechessai_amd.replay import ReplayBuffer
    models = _models(SEEDS, S, 0.25, 16)
    eng = _engine(len(SEEDS))
    buf = ReplayBuffer(max_size=64 * 70)
    try:
        eng.set_playout_cap(0.25, 16, seed=CAP_SEED)
        eng.play(HashNetEvaluator(), SEEDS, read=False)
        t, rec = _pack(eng, len(SEEDS))
        want = [(g, i) for g, m in enumerate(models) for i in range(m.n_samples) if m.full[i]]
        assert buf.push_records(t, len(SEEDS)) == len(want) == len(buf)
        idx = np.arange(len(want), dtype=np.int64)
        got = np.zeros(len(want), dtype=RECORD_DTYPE)
        buf._chk(buf.L.xq_replay_read_records(buf.h, C.c_void_p(buf._stream()), _lib.ptr(idx), len(idx), _lib.ptr(got)))
        assert got.tobytes() == rec[[g for g, _ in want], [i for _, i in want]].tobytes()
        assert got["valid"].all() and not got["pad"].any()
        _, _, target = buf.sample_policy_tensors(len(want), indices=idx)
        pi, n_moves = target.pi.cpu().numpy(), target.n_moves.cpu().numpy()
        for k, (g, i) in enumerate(want):
            m = models[g]
            n = len(m.moves[i])
            assert int(n_moves[k]) == n and pi[k, :n].tobytes() == m.pi[i].astype(np.float32).tobytes(), (g, i)
            assert not pi[k, n:].any()
    finally:
        buf.close()
        eng.close()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable(L):
    """Virtual loss, tree reuse, the two-network calls, a pairing-1 game and opponent-mode engines refuse the cap, whichever
    call comes first; fast_sims <= leaf_batch and > sims are refused; each refusal carries a message and the engine plays
    on afterwards."""
    import torch
    from chinesechessai_amd import _lib, distributed as xd
    from chinesechessai_amd.engine import HashNetEvaluator
    G = 8
    seeds = SEEDS[:G]

    def refused(fn, word):
        with pytest.raises(_lib.XqError) as ei:
            fn()
        assert word in str(ei.value), str(ei.value)

    def still_plays(eng, capped):
        b = eng.play(HashNetEvaluator(), seeds)
        assert int(b.error.sum()) == 0 and (b.n_plies > 0).all()
        ps = eng.ply_sims()
        assert ((ps == 16).any() and (ps == S).any()) if capped else set(np.unique(ps)) <= {0, S}

    eng = _engine(G)
    try:
        # the cap first, then the other switch
        eng.set_playout_cap(0.25, 16, seed=CAP_SEED)
        refused(lambda: eng.set_virtual_loss(True), "playout cap")
        refused(lambda: eng.set_tree_reuse(True), "playout cap")
        refused(lambda: eng.set_pairing(np.ones(G, np.uint8)), "playout cap")
        pp, vp = eng.priors_ptr, eng.values_ptr
        refused(lambda: _lib.check(eng.L.xq_engine_search_round2(eng.h, 0, 0, None, None, 0, None, None, None)), "playout cap")
        refused(lambda: _lib.check(eng.L.xq_engine_end_search2(eng.h, 0, pp, vp, 0, pp, vp)), "playout cap")
        rec_t = torch.zeros(2 * G * 70 * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
        two = np.arange(7000, 7000 + 2 * G, dtype=np.uint32)
        refused(lambda: _lib.check(eng.L.xq_engine_refill_begin2(eng.h, _lib.ptr(two), 2 * G, _lib.ptr(np.ones(2 * G, np.uint8)))),
                "playout cap")
        refused(lambda: eng.play_refill(HashNetEvaluator(0), two, rec_t.data_ptr(), opponent_evaluator=HashNetEvaluator(1)),
                "playout cap")
        refused(lambda: eng.play(HashNetEvaluator(0), seeds, opponent_evaluator=HashNetEvaluator(1)), "playout cap")
        # bad budgets (the cap stays as it was)
        for bad in (LB, LB - 1, 1, S + 1, -3):
            refused(lambda: eng.set_playout_cap(0.25, bad), "fast_sims")
        for bad in (0.0, -0.1, 1.5, float("nan")):
            refused(lambda: eng.set_playout_cap(bad, 16), "full_prob")
        still_plays(eng, True)
        # the other switch first, then the cap
        eng.set_playout_cap(1.0, 0)
        eng.set_virtual_loss(True)
        refused(lambda: eng.set_playout_cap(0.25, 16), "virtual loss")
        eng.set_virtual_loss(False)
        eng.set_tree_reuse(True)
        refused(lambda: eng.set_playout_cap(0.25, 16), "tree reuse")
        eng.set_tree_reuse(False)
        eng.set_pairing(np.ones(G, np.uint8))
        refused(lambda: eng.set_playout_cap(0.25, 16), "second network")
        eng.set_pairing(np.zeros(G, np.uint8))
        eng.new_games(seeds)
        _lib.check(eng.L.xq_engine_search_round2(eng.h, 0, 0, None, None, 0, None, None, None))
        refused(lambda: eng.set_playout_cap(0.25, 16), "second network")
        still_plays(eng, False)
        eng.set_playout_cap(0.25, 16, seed=CAP_SEED)                          # (new games: no two-network round in flight)
        still_plays(eng, True)
    finally:
        eng.close()
    opp = _engine(G, opponent_mode=True)
    try:
        refused(lambda: opp.set_playout_cap(0.25, 16), "second network")
        b = opp.play(HashNetEvaluator(0), seeds, opponent_evaluator=HashNetEvaluator(1))
        assert int(b.error.sum()) == 0
    finally:
        opp.close()


# ---- 10. the switch set while games are in the slots ----------------------------------------------------------------------
def test_plies_stored_before_the_switch_count_as_full(L):
    """Five plies without the cap, then the switch: the stored plies were searched with `sims` and are reported and packed
    as full plies (pad = 0, valid = 1); from the sixth ply on budgets follow the plan."""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import HashNetEvaluator, playout_plan
    G, before, after = len(SEEDS), 5, 6
    full = playout_plan(np.stack([pm.game_uniforms(s) for s in SEEDS]), CAP_SEED, 0.25)
    eng = _engine(G)
    try:
        ev = HashNetEvaluator()
        ev.bind(eng)
        eng.new_games(SEEDS)
        for ply in range(before + after):
            if ply == before:
                eng.set_playout_cap(0.25, 16, seed=CAP_SEED)
            eng.search(ev)
            _, visits, _ = eng.root_visits()
            want = np.full(G, S) if ply < before else np.where(full[:, ply], S, 16)
            assert np.array_equal(visits.sum(axis=1), want - LB), ply
            _lib.check(eng.L.xq_engine_play_move(eng.h))
        ps = eng.ply_sims()
        _, rec = _pack(eng, G)
    finally:
        eng.close()
    n = before + after
    want = np.concatenate([np.full((G, before), S), np.where(full[:, before:n], S, 16)], axis=1)
    assert np.array_equal(ps[:, :n], want) and not ps[:, n:].any()
    assert np.array_equal(rec["pad"][:, :n], (want != S).astype(np.uint8)) and not rec["pad"][:, n:].any()
    assert np.array_equal(rec["valid"][:, :n], (want == S).astype(np.uint8)) and not rec["valid"][:, n:].any()
    assert (want[:, before:] == 16).any()
