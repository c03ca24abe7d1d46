"""Two networks chosen per slot on the device (`-m gpu`): the reference trainer's "new model red vs frozen old model black"
games (trainer.py:186-209, self_play.py:190-198, 211, 234) through the refill pool, mixed with self-play games, with slots
at different plies - xq_engine_search_round2 / end_search2 / refill_begin2 / set_pairing / row_map_net / eval_hashnet2
behind SelfPlayEngine.search(per_slot=True), play_refill(opponent_evaluator=, pairing=) and self_play_epoch."""
import struct

import numpy as np
import pytest

from tests.test_gpu_round4 import _mate_line_net, _same_game
from tests.test_oracle_search import _salted

pytestmark = pytest.mark.gpu

SEEDS = np.array([503, 0, 1, 3, 503, 5, 943, 6], dtype=np.uint32)
S = 50


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


@pytest.fixture(scope="module")
def oracle_games():
    """the CPU oracle's game of every seed, once: [pairing][seed] (pairing 1 = HashNet(0) red vs HashNet(1) black)"""
    from oracle import xq_oracle as xo
    games = {0: {}, 1: {}}
    for seed in sorted(set(int(s) for s in SEEDS)):
        rc, g = xo.self_play_game(seed, S)
        assert rc == 0
        games[0][seed] = g
        rc, g = xo.self_play_game(seed, S, eval_black=_salted(1))
        assert rc == 0
        games[1][seed] = g
    # the early ending the schedule relies on (measured with the oracle: seed 503 vs salt 1 ends at ply 35, red wins)
    g = games[1][503]
    assert (g.n_plies, g.winner, g.n_samples) == (35, 1, 18)
    g = games[1][943]
    assert (g.n_plies, g.winner, g.n_samples) == (50, -1, 25)
    return games


def _refill_hashnet_pair(pairing):
    """SEEDS through 4 slots with HashNet(0) / HashNet(1): (outcomes, records [T][70], [(ply, slot ids)])"""
    import torch
    from chinesechessai_amd import distributed as xd
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    T = len(SEEDS)
    eng = SelfPlayEngine(4, sims=S)
    rec_t = torch.zeros(T * 70 * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    seen = []
    out, plies = eng.play_refill(HashNetEvaluator(0), SEEDS, rec_t.data_ptr(), check_every=1,
                                 on_ply=lambda ply: seen.append((ply, eng.refill_slots())),
                                 opponent_evaluator=HashNetEvaluator(1), pairing=pairing)
    rec = xd.records_to_numpy(rec_t).reshape(T, 70)
    eng.close()
    assert len(seen) == plies
    return out, rec, seen


def _equals_oracle_game(out, rec, i, og, red_only):
    """game i of a refill session against the oracle's game: outcome, and every stored record bit for bit"""
    assert (out["winner"][i], out["reason"][i], out["n_plies"][i], out["n_samples"][i]) == (
        og.winner, og.end_reason, og.n_plies, og.n_samples), (i, red_only)
    assert out["error"][i] == 0
    assert int(rec[i]["valid"].sum()) == og.n_samples and rec[i]["valid"][:og.n_samples].all()
    for j in range(og.n_samples):
        ply = 2 * j if red_only else j                        # the oracle's per-ply trace (t_*) against per-sample records
        k = og.s_nmoves[j]
        assert int(rec[i, j]["n_moves"]) == k and int(rec[i, j]["player"]) == og.s_player[j], (i, j)
        assert rec[i, j]["moves"][:k].tolist() == list(og.s_moves[j][:k]), (i, j)
        assert rec[i, j]["counts"][:k].tolist() == list(og.t_visits[ply][:k]), (i, j)
        assert int(rec[i, j]["chosen"]) == og.t_move[j], (i, j)               # (`chosen` is indexed by ply in every mode)
        assert struct.pack("<d", og.s_z[j]) == struct.pack("<d", float(rec[i, j]["z"])), (i, j)
    if red_only:
        assert all(int(p) == 1 for p in rec[i]["player"][:og.n_samples])


def _restart_plies(seen, n_slots):
    """(ply, slot) of every restart: the slot holds another game after the step of `ply` than before it"""
    prev = np.arange(n_slots)
    out = []
    for ply, slots in seen:
        for s in np.nonzero((slots != prev) & (slots >= 0))[0]:
            out.append((ply + 1, int(s)))                     # the new game's first ply is searched at step ply + 1
        prev = slots
    return out


def test_opponent_games_through_refill_equal_the_oracle_with_slots_out_of_parity(L, oracle_games):
    """Issue test 1.  8 games, all "HashNet(0) red vs HashNet(1) black", through 4 slots at S = 50.  Seed 503 ends at ply
    35: slot 0 restarts at an ODD step and is red-to-move while its neighbours are black-to-move for the next 35 plies -
    the host cannot pick the network by ply number.  Every game, in whatever slot, must be the oracle's game of its seed."""
    out, rec, seen = _refill_hashnet_pair(None)                  # (no pairing given + an opponent: all 1)
    for i, seed in enumerate(SEEDS):
        _equals_oracle_game(out, rec, i, oracle_games[1][int(seed)], True)
    restarts = _restart_plies(seen, 4)
    assert (35, 0) in restarts, restarts                          # slot 0, after game 0's 35 plies
    assert any(p % 2 == 1 for p, _ in restarts)


def test_mixed_pairing_through_refill_equals_the_oracle(L, oracle_games):
    """Issue test 2.  The same seeds and slots, pairing alternating 0 / 1 by game id: self-play games keep both sides'
    samples and equal the single-network oracle game, the others equal test 1's."""
    pairing = (np.arange(len(SEEDS)) % 2).astype(np.uint8)
    out, rec, seen = _refill_hashnet_pair(pairing)
    for i, seed in enumerate(SEEDS):
        _equals_oracle_game(out, rec, i, oracle_games[int(pairing[i])][int(seed)], bool(pairing[i]))
    assert out["n_samples"][0] == 70 and out["n_samples"][1] == oracle_games[1][0].n_samples


def _roots_after_one_red_move():
    """8 roots, black to move: [X] * 4 + [Y] * 4, X / Y = the start position after the cannon move (7,1)->(7,4) / the
    pawn move (6,0)->(5,0)"""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.chess_env import ChineseChess
    start = np.ascontiguousarray(ChineseChess().board, dtype=np.int8).reshape(90)
    boards = []
    for fr, to in ((7 * 9 + 1, 7 * 9 + 4), (6 * 9 + 0, 5 * 9 + 0)):
        b = start.copy()
        assert b[fr] > 0 and b[to] == 0
        b[to], b[fr] = b[fr], 0
        boards += [b] * 4
    st = np.zeros((8, _lib.STATE_WORDS), np.int32)
    st[:, _lib.S_PLAYER] = -1
    st[:, _lib.S_MOVE_COUNT] = 1
    st[:, _lib.S_WINNER] = _lib.WINNER_NONE
    st[:, _lib.S_RED_KING] = 9 * 9 + 4
    st[:, _lib.S_BLACK_KING] = 4
    st[:, _lib.S_NO_CAPTURE] = 1
    return np.stack(boards), st


def _trees(eng):
    moves, visits, n = eng.root_visits()
    return [(moves[g].tolist(), visits[g].tolist(), int(n[g]), eng.read_tree(g)) for g in range(eng.n_games)]


def _same_tree(a, b, ctx):
    assert a[:3] == b[:3], ctx
    for k in ("visit_count", "value_sum", "prior", "move", "first_child", "n_child"):
        assert a[3][k].tobytes() == b[3][k].tobytes(), (ctx, k)
    assert a[3]["root"] == b[3]["root"], ctx


@pytest.mark.parametrize("dedupe", [True, False])
def test_leaf_dedupe_never_crosses_networks(L, dedupe):
    """Issue test 3.  Two bf16 networks with different weights; 8 black-to-move roots [X]*4 + [Y]*4 with pairing
    [0,1]*4: in round 0 the even slots wait for network 0 and the odd slots - the SAME two positions - for network 1.
    One per-slot search must give every even slot the tree of a single-network search with network 0 and every odd slot
    that of network 1, bit for bit; with the dedupe on round 0 has exactly 2 rows per network (X and Y, once each), with
    it off 4 and 4."""
    import torch
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    boards, st = _roots_after_one_red_move()
    nets = []
    for seed in (21, 22):
        torch.manual_seed(seed)
        nets.append(ChessNet(num_blocks=1).eval().cuda())
    evs = [TorchNetEvaluator(n, leaf_dedupe=dedupe, eval_cache=False) for n in nets]

    single = []
    for ev in evs:                                            # the existing path: one network for every slot
        eng = SelfPlayEngine(8, sims=16, planes_format=ev.planes_format)
        eng.set_root_eval_carry(False)
        eng._bind(ev)
        eng.set_roots(boards, st)
        eng.search(ev)
        single.append(_trees(eng))
        eng.close()
    assert single[0][0][3]["prior"].tobytes() != single[1][0][3]["prior"].tobytes()       # the networks do differ

    eng = SelfPlayEngine(8, sims=16, planes_format=evs[0].planes_format)
    eng.set_root_eval_carry(False)
    eng._bind(evs[0], evs[1], per_slot=True)
    assert eng.leaf_dedupe == dedupe and eng.row_compaction and not eng.eval_cache
    eng.set_roots(boards, st)
    eng.set_pairing([0, 1] * 4)
    n_before = eng.row_history(cap=0)[1]
    eng.search(evs[0], evs[1], per_slot=True)
    got = _trees(eng)
    R = eng.rounds
    rows0, n0 = eng.row_history_net(0, cap=R)
    rows1, n1 = eng.row_history_net(1, cap=R)
    total, n = eng.row_history(cap=R)
    eng.close()
    for g in range(8):
        _same_tree(got[g], single[g % 2][g], (g, dedupe))
    assert n0 == n1 == n == n_before + R
    assert (rows0[0], rows1[0]) == ((2, 2) if dedupe else (4, 4)), (rows0, rows1)
    assert (rows0 + rows1 == total).all()


def _real_network_reference(netA, netB, seeds_even, seeds_odd, sims):
    """the existing plain lock-step paths: play(evA) for the self-play games, an opponent-mode engine's
    play(evA, opponent_evaluator=evB) for the others: (records, outcomes) of each"""
    import torch
    from chinesechessai_amd import distributed as xd
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    res = []
    for seeds, opp in ((seeds_even, False), (seeds_odd, True)):
        evA = TorchNetEvaluator(netA, leaf_dedupe=False, eval_cache=False)
        evB = TorchNetEvaluator(netB, leaf_dedupe=False, eval_cache=False) if opp else None
        eng = SelfPlayEngine(len(seeds), sims=sims, planes_format=evA.planes_format, opponent_mode=opp)
        eng.set_root_eval_carry(False)
        eng.play(evA, seeds, opponent_evaluator=evB, read=False)
        t = torch.zeros(len(seeds) * 70 * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
        eng.pack_samples(t.data_ptr())
        out = eng.read_game_outcomes()
        eng.close()
        assert int(out["error"].sum()) == 0
        res.append((xd.records_to_numpy(t).reshape(len(seeds), 70), out))
    return res


def test_real_networks_mixed_refill_equals_lock_step(L):
    """Issue test 4.  A = _mate_line_net(2, 11), B = _mate_line_net(2, 12); 48 games through 16 slots at S = 50, pairing
    0 for even ids and 1 for odd ids, leaf dedupe on and off.  Every game's records equal the existing lock-step paths'
    (play(evA) for the even ids, an opponent-mode engine's play(evA, opponent_evaluator=evB) for the odd ids), outcomes
    are equal and the guard blocks around the record buffer are untouched.  The opponent games must really put slots
    out of parity: at least 3 of the 24 lock-step opponent games have odd length and refill restarts happen at odd
    plies (both asserted).  Counts: with the CPU oracle and the two networks as fp32
    callbacks, 3 of the 24 opponent games end at ply 7 and 21 at the 70-ply cap (seed 13 for B gives the same 3 / 21); on
    an MI355X with the bf16 kernels the lock-step reference gives the same lengths (3 games of odd length: 7, 7, 7) and 8
    of the session's 32 restarts fall on odd plies."""
    import torch
    from chinesechessai_amd import distributed as xd
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    G, T = 16, 48
    netA, netB = _mate_line_net(2, 11), _mate_line_net(2, 12)
    seeds = (np.arange(T, dtype=np.uint32) * 7 + 3).astype(np.uint32)
    pairing = (np.arange(T) % 2).astype(np.uint8)
    (ref0, out0), (ref1, out1) = _real_network_reference(netA, netB, seeds[0::2], seeds[1::2], S)
    odd_games = int((out1["n_plies"] % 2 == 1).sum())
    print("opponent games of odd length:", odd_games, sorted(out1["n_plies"].tolist()))
    assert odd_games >= 3, sorted(out1["n_plies"].tolist())
    assert (out1["n_samples"] == (out1["n_plies"] + 1) // 2).all() and (out0["n_samples"] == out0["n_plies"]).all()

    block = 70 * xd.RECORD_BYTES
    for dedupe in (True, False):
        evA = TorchNetEvaluator(netA, leaf_dedupe=dedupe)
        evB = TorchNetEvaluator(netB, leaf_dedupe=dedupe)
        eng = SelfPlayEngine(G, sims=S, planes_format=evA.planes_format)
        buf = torch.full(((T + 2) * block,), 0xA5, dtype=torch.uint8, device="cuda")
        seen = []
        out, plies = eng.play_refill(evA, seeds, buf.data_ptr() + block, check_every=1,
                                     on_ply=lambda ply, eng=eng, seen=seen: seen.append((ply, eng.refill_slots())),
                                     opponent_evaluator=evB, pairing=pairing)
        assert not eng._carry_on and not eng.eval_cache and eng.row_compaction and eng.leaf_dedupe == dedupe
        eng.close()
        host = buf.cpu().numpy()
        assert (host[:block] == 0xA5).all() and (host[-block:] == 0xA5).all()              # guard blocks
        rec = np.frombuffer(host[block:-block].tobytes(), dtype=xd.RECORD_DTYPE).reshape(T, 70)
        for k in ("winner", "reason", "reason_side", "reason_count", "n_plies", "n_samples", "error"):
            assert np.array_equal(out[k][0::2], out0[k]), (k, dedupe)
            assert np.array_equal(out[k][1::2], out1[k]), (k, dedupe)
        for g in range(T):
            _same_game(rec[g], (ref1 if g % 2 else ref0)[g // 2], (g, dedupe))
        restarts = _restart_plies(seen, G)
        odd_restarts = sum(1 for p, _ in restarts if p % 2 == 1)
        print("restarts at odd plies:", odd_restarts, "of", len(restarts))
        assert odd_restarts >= 1, restarts


def test_self_play_epoch_is_the_trainers_mix_in_one_session(L):
    """Issue test 5a.  self_play_epoch with a HashNet pair, 6 games through 4 slots: the first 3 results hold samples of
    both players, the last 3 red plies only, and each result equals parallel_self_play's for the same seed - without
    the opponent for the first half, with it for the second - {move: prob} and z bit for bit."""
    from chinesechessai_amd.engine import HashNetEvaluator
    from chinesechessai_amd.self_play import parallel_self_play, self_play_epoch
    seeds = np.array([11, 12, 13, 503, 15, 16], dtype=np.uint32)
    got = self_play_epoch(HashNetEvaluator(0), 6, 1.0, S, opponent_network=HashNetEvaluator(1), slots=4, seeds=seeds)
    assert len(got) == 6
    ref = parallel_self_play(HashNetEvaluator(0), 3, 1.0, S, seeds=seeds[:3]) + \
        parallel_self_play(HashNetEvaluator(0), 3, 1.0, S, opponent_network=HashNetEvaluator(1), seeds=seeds[3:])
    from oracle import xq_oracle as xo
    for g in range(6):
        (da, wa, ra), (db, wb, rb) = got[g], ref[g]
        assert (wa, ra) == (wb, rb) and len(da) == len(db), g
        rc, og = xo.self_play_game(int(seeds[g]), S, eval_black=_salted(1) if g >= 3 else None)
        players = [int(og.s_player[i]) for i in range(og.n_samples)]
        assert len(da) == og.n_samples
        assert set(players) == ({1} if g >= 3 else {1, -1}), g
        for (ba, pa, za), (bb, pb, zb) in zip(da, db):
            assert np.array_equal(ba, bb) and list(pa) == list(pb), g
            assert [struct.pack("<d", x) for x in pa.values()] == [struct.pack("<d", x) for x in pb.values()], g
            assert struct.pack("<d", za) == struct.pack("<d", zb), g
    # without an opponent: all self-play
    solo = self_play_epoch(HashNetEvaluator(0), 2, 1.0, 16, slots=2, seeds=seeds[:2])
    ref = parallel_self_play(HashNetEvaluator(0), 2, 1.0, 16, seeds=seeds[:2])
    assert [(w, r, len(d)) for d, w, r in solo] == [(w, r, len(d)) for d, w, r in ref]


def test_play_sharded_with_an_opponent_network_one_rank(L):
    """Issue test 5b.  play_sharded(..., opponent_network=B) under RCCL with the one rank a GPU box offers: both networks
    are broadcast (one broadcast_weights each) and the shard is played with both; records and outcomes equal the local
    two-network run of the same seeds."""
    import os
    import socket
    import torch
    import torch.distributed as dist
    from chinesechessai_amd import distributed as xd
    G, sims = 8, 16
    netA, netB = _mate_line_net(1, 31), _mate_line_net(1, 32)
    if dist.is_initialized():
        dist.destroy_process_group()
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        out, gathered = xd.play_sharded(None, G, sims, base_seed=5, network=netA, opponent_network=netB)
        rec = xd.records_to_numpy(gathered).reshape(G, 70)
    finally:
        dist.destroy_process_group()
    _, (ref, ref_out) = _real_network_reference(netA, netB, xd.game_seeds(5, G, 0, 1), xd.game_seeds(5, G, 0, 1), sims)
    for k in ref_out:
        assert np.array_equal(out[k], ref_out[k]), k
    for g in range(G):
        _same_game(rec[g], ref[g], g)
    assert (out["n_samples"] == (out["n_plies"] + 1) // 2).all()
