"""The root evaluation carry-over and the evaluation cache in two-network sessions (`-m gpu`):
xq_engine_set_per_slot_reuse behind SelfPlayEngine.set_per_slot_reuse, play_refill(reuse=True) and
self_play_epoch(reuse=True).  The carry-over is decided per slot (pairing 0 only), the cache's key carries the leaf's
network, and its window is three plies where two networks alternate.  Everything here fails without the feature at its
first call: the entry point does not exist and the combinations are refused."""
import struct

import numpy as np
import pytest

from tests.test_gpu_round4 import _mate_line_net, _same_game
from tests.test_gpu_two_networks import (SEEDS, S, _equals_oracle_game, _restart_plies, _roots_after_one_red_move, _same_tree,
                                         _trees, oracle_games)  # noqa: F401  (oracle_games: a fixture)

pytestmark = pytest.mark.gpu

G2, T2 = 16, 48                      # test 2: 48 games through 16 slots


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


def test_carry_per_slot_equals_the_oracle(L, oracle_games):
    """Issue test 1.  HashNet(0) / HashNet(1), the eight SEEDS through 4 slots at S = 50, pairing 0 / 1 alternating by
    game id, reuse=True with the carry-over on.  Every game is its oracle game (red plies only for pairing 1), and after
    every step roots_not_ready() = occupied slots holding a pairing-1 game + pairing-0 slots restarted in that step: a
    carried pairing-1 root or an uncarried continuing pairing-0 root both break the count."""
    import torch
    from chinesechessai_amd import distributed as xd
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    T = len(SEEDS)
    pairing = (np.arange(T) % 2).astype(np.uint8)
    eng = SelfPlayEngine(4, sims=S)
    eng.set_root_eval_carry(True)                 # (by-slot evaluators get it by this call only)
    rec_t = torch.zeros(T * 70 * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    seen = []
    out, plies = eng.play_refill(HashNetEvaluator(0), SEEDS, rec_t.data_ptr(), check_every=1,
                                 on_ply=lambda ply: seen.append((eng.refill_slots(), eng.roots_not_ready())),
                                 opponent_evaluator=HashNetEvaluator(1), pairing=pairing, reuse=True)
    assert eng._carry_on and eng._slot_reuse
    rec = xd.records_to_numpy(rec_t).reshape(T, 70)
    eng.close()
    for i, seed in enumerate(SEEDS):
        _equals_oracle_game(out, rec, i, oracle_games[int(pairing[i])][int(seed)], bool(pairing[i]))
    assert len(seen) == plies
    prev = np.arange(4)
    carried = 0
    for p, (slots, not_ready) in enumerate(seen):
        occupied = slots >= 0
        restarted = (slots != prev) & occupied
        pair1 = np.zeros(4, bool)
        pair1[occupied] = pairing[slots[occupied]] == 1
        want = int(pair1.sum()) + int((restarted & ~pair1).sum())
        assert not_ready == want, (p, slots.tolist(), not_ready, want)
        carried += int((occupied & ~pair1 & ~restarted).sum())
        prev = slots
    assert carried > 100 and any(n > 0 for _, n in seen)       # both kinds of slot were there


def _play_mixed(netA, netB, seeds, pairing, dedupe, cache, reuse, slots=G2, keep_plies=None):
    """one play_refill of the two real networks: (outcomes, records, plies, seen slots per step, engine facts)"""
    import torch
    from chinesechessai_amd import distributed as xd
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    T = len(seeds)
    block = 70 * xd.RECORD_BYTES
    evA = TorchNetEvaluator(netA, leaf_dedupe=dedupe, eval_cache=cache)
    evB = TorchNetEvaluator(netB, leaf_dedupe=dedupe, eval_cache=cache)
    eng = SelfPlayEngine(slots, sims=S, planes_format=evA.planes_format)
    eng.reuse_keep_plies = keep_plies
    buf = torch.full(((T + 2) * block,), 0xA5, dtype=torch.uint8, device="cuda")
    seen = []
    out, plies = eng.play_refill(evA, seeds, buf.data_ptr() + block, check_every=1,
                                 on_ply=lambda ply: seen.append(eng.refill_slots()),
                                 opponent_evaluator=evB, pairing=pairing, reuse=reuse)
    R = eng.rounds
    facts = dict(carry=eng._carry_on, cache=eng.eval_cache, dedupe=eng.leaf_dedupe, stats=eng.eval_cache_stats(), rounds=R,
                 rows0=eng.row_history_net(0)[0].copy(), rows1=eng.row_history_net(1)[0].copy())
    eng.close()
    host = buf.cpu().numpy()
    assert (host[:block] == 0xA5).all() and (host[-block:] == 0xA5).all()              # guard blocks
    rec = np.frombuffer(host[block:-block].tobytes(), dtype=xd.RECORD_DTYPE).reshape(T, 70)
    assert len(seen) == plies
    return out, rec, plies, seen, facts


@pytest.fixture(scope="module")
def mixed_reference(L):
    """the plain path, once: the same session with reuse=False (no carry-over, no cache), and the two networks"""
    netA, netB = _mate_line_net(2, 11), _mate_line_net(2, 12)
    seeds = (np.arange(T2, dtype=np.uint32) * 7 + 3).astype(np.uint32)
    pairing = (np.arange(T2) % 2).astype(np.uint8)
    out, rec, plies, seen, facts = _play_mixed(netA, netB, seeds, pairing, True, True, False)
    assert not facts["carry"] and not facts["cache"]
    assert int(out["error"].sum()) == 0
    return netA, netB, seeds, pairing, out, rec


@pytest.mark.parametrize("cache", [True, "verify"])
@pytest.mark.parametrize("dedupe", [True, False])
def test_real_networks_with_reuse_equal_the_plain_session(L, mixed_reference, dedupe, cache):
    """Issue test 2.  A = _mate_line_net(2, 11), B = _mate_line_net(2, 12), 48 games through 16 slots at S = 50, pairing
    even 0 / odd 1.  With reuse=True - carry-over in the self-play slots, one cache for both networks - every game's
    records and all outcomes equal the same session's with reuse=False, the guard blocks around the record buffer are
    untouched, and in verify mode the cache never disagrees with a fresh evaluation while it does answer.  A key without
    the network would hand B the answer A gave for the root of every black ply: mismatches from the first black ply on."""
    netA, netB, seeds, pairing, ref_out, ref = mixed_reference
    out, rec, plies, seen, facts = _play_mixed(netA, netB, seeds, pairing, dedupe, cache, True)
    assert facts["carry"] and facts["cache"] and facts["dedupe"] == dedupe
    for k in ("winner", "reason", "reason_side", "reason_count", "n_plies", "n_samples", "error"):
        assert np.array_equal(out[k], ref_out[k]), (k, dedupe, cache)
    for g in range(T2):
        _same_game(rec[g], ref[g], (g, dedupe, cache))
    hits, fills, mismatches = facts["stats"]
    print("dedupe %s cache %s: hits %d fills %d mismatches %d, rows %d + %d" % (
        dedupe, cache, hits, fills, mismatches, int(facts["rows0"].sum()), int(facts["rows1"].sum())))
    if cache == "verify":
        assert mismatches == 0 and hits > 0, facts["stats"]


def test_round_0_rows_of_a_reuse_session(L, mixed_reference):
    """Issue test 2, last run: cache and dedupe off, so every pending leaf is a row.  Round 0 of a ply then has exactly
    these rows - network 0: the slots restarted in the step before plus the pairing-1 slots with red to move; network 1:
    the pairing-1 slots with black to move - and none for a continuing pairing-0 slot (its root was carried over)."""
    netA, netB, seeds, pairing, ref_out, ref = mixed_reference
    out, rec, plies, seen, facts = _play_mixed(netA, netB, seeds, pairing, False, False, True)
    assert facts["carry"] and not facts["cache"] and not facts["dedupe"]
    for k in ref_out:
        assert np.array_equal(out[k], ref_out[k]), k
    for g in range(T2):
        _same_game(rec[g], ref[g], g)
    R = facts["rounds"]
    assert len(facts["rows0"]) == plies * R == len(facts["rows1"])
    per0, per1 = facts["rows0"].reshape(plies, R), facts["rows1"].reshape(plies, R)
    assert (per0[0, 0], per1[0, 0]) == (G2, 0)                 # the first ply: every slot is a fresh game, red to move
    prev, played = np.arange(G2), np.zeros(G2, int)
    continuing0 = 0
    for p, slots in enumerate(seen):
        occupied = slots >= 0
        restarted = (slots != prev) & occupied
        played = np.where(restarted, 0, played + 1)            # plies the slot's game has played after this step
        pair1 = np.zeros(G2, bool)
        pair1[occupied] = pairing[slots[occupied]] == 1
        cont1 = occupied & ~restarted & pair1
        want0 = int(restarted.sum()) + int((cont1 & (played % 2 == 0)).sum())
        want1 = int((cont1 & (played % 2 == 1)).sum())
        continuing0 += int((occupied & ~restarted & ~pair1).sum())
        if p + 1 < plies:
            assert (per0[p + 1, 0], per1[p + 1, 0]) == (want0, want1), (p, slots.tolist(), per0[p + 1, 0], per1[p + 1, 0])
        prev = slots
    assert continuing0 > 1000                                   # ... of which there were plenty
    assert len(_restart_plies([(p, s) for p, s in enumerate(seen)], G2)) >= 3


def test_the_three_ply_window(L, mixed_reference):
    """Issue test 3.  One slot, one pairing-1 game (seed 0), the same two networks, S = 50, verify mode, once with a
    two-ply and once with a three-ply window.  Records equal the reuse=False run both times and nothing mismatches;
    the three-ply window answers more: with one game there is nobody to transpose with, so the difference is network A
    meeting its own evaluations from two plies back.  Seed chosen on the CPU (the oracle with the two networks as fp32
    callbacks): of the 236 leaf evaluations of A's 35 plies in that game, 188 are positions A evaluated two plies
    earlier (31 of them roots); all of seeds 0..31 give at least 13."""
    netA, netB = mixed_reference[0], mixed_reference[1]
    seeds, pairing = np.array([0], np.uint32), np.array([1], np.uint8)
    ref_out, ref, _, _, facts = _play_mixed(netA, netB, seeds, pairing, True, "verify", False, slots=1)
    assert not facts["cache"] and not facts["carry"]
    hits = {}
    for keep in (2, 3):
        out, rec, _, _, facts = _play_mixed(netA, netB, seeds, pairing, True, "verify", True, slots=1, keep_plies=keep)
        assert facts["cache"]
        for k in ref_out:
            assert np.array_equal(out[k], ref_out[k]), (k, keep)
        _same_game(rec[0], ref[0], keep)
        hits[keep], fills, mismatches = facts["stats"]
        assert mismatches == 0, (keep, facts["stats"])
        print("keep_plies %d: hits %d fills %d" % (keep, hits[keep], fills))
    assert hits[3] > hits[2], hits


def test_lock_step_form_and_the_refusals_that_stay(L, mixed_reference):
    """Issue test 4.  Four identical black-to-move roots, set_pairing([0, 1, 0, 1]), A / B bound per slot, cache on,
    carry-over off: two plies of search(per_slot=True) + play_move give every slot the tree, node by node, of the run
    with set_per_slot_reuse(False) and no cache, and the cache was filled.  Without the switch the refusals are
    today's; with it an opponent-mode engine still refuses the carry-over."""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine, TorchNetEvaluator
    netA, netB = mixed_reference[0], mixed_reference[1]
    boards, st = _roots_after_one_red_move()
    boards, st = boards[:4], st[:4]
    uniforms = np.random.RandomState(7).random_sample((4, 70))

    def run(reuse):
        evA = TorchNetEvaluator(netA, eval_cache=reuse)
        evB = TorchNetEvaluator(netB, eval_cache=reuse)
        eng = SelfPlayEngine(4, sims=S, planes_format=evA.planes_format)
        eng.set_root_eval_carry(False)
        eng.set_per_slot_reuse(reuse)
        eng._bind(evA, evB, per_slot=True)
        assert eng.eval_cache == reuse
        eng.set_roots(boards, st)
        eng.set_pairing([0, 1, 0, 1])
        eng.set_uniforms(uniforms)
        trees = []
        for ply in range(2):
            eng.search(evA, evB, per_slot=True)
            trees.append(_trees(eng))
            _lib.check(eng.L.xq_engine_play_move(eng.h))
        stats = eng.eval_cache_stats()
        eng.close()
        return trees, stats

    plain, _ = run(False)
    got, (hits, fills, mismatches) = run(True)
    for ply in range(2):
        for g in range(4):
            _same_tree(got[ply][g], plain[ply][g], (ply, g))
    assert plain[0][0][3]["prior"].tobytes() != plain[0][1][3]["prior"].tobytes()        # the two networks do differ
    assert fills > 0, (hits, fills)

    eng = SelfPlayEngine(4, sims=16)
    eng.set_eval_cache(True)
    with pytest.raises(_lib.XqError):
        eng.set_pairing([0, 1, 0, 1])
    eng.close()
    eng = SelfPlayEngine(4, sims=16)
    eng.set_root_eval_carry(True)
    eng.new_games(np.arange(4, dtype=np.uint32))
    with pytest.raises(_lib.XqError):
        eng.search(HashNetEvaluator(0), HashNetEvaluator(1), per_slot=True)
    eng.close()
    eng = SelfPlayEngine(4, sims=16, opponent_mode=True)
    eng.set_per_slot_reuse(True)
    with pytest.raises(_lib.XqError):
        eng.set_root_eval_carry(True)
    eng.close()


def test_self_play_epoch_with_reuse(L):
    """Issue test 5.  self_play_epoch(..., reuse=True) with the HashNet pair, 6 games through 4 slots: the same results
    as reuse=False, {move: prob} and z bit for bit."""
    from chinesechessai_amd.engine import HashNetEvaluator
    from chinesechessai_amd.self_play import self_play_epoch
    seeds = np.array([11, 12, 13, 503, 15, 16], dtype=np.uint32)
    got = self_play_epoch(HashNetEvaluator(0), 6, 1.0, S, opponent_network=HashNetEvaluator(1), slots=4, seeds=seeds, reuse=True)
    ref = self_play_epoch(HashNetEvaluator(0), 6, 1.0, S, opponent_network=HashNetEvaluator(1), slots=4, seeds=seeds)
    assert len(got) == len(ref) == 6
    for g in range(6):
        (da, wa, ra), (db, wb, rb) = got[g], ref[g]
        assert (wa, ra) == (wb, rb) and len(da) == len(db), g
        for (ba, pa, za), (bb, pb, zb) in zip(da, db):
            assert np.array_equal(ba, bb) and list(pa) == list(pb), g
            assert [struct.pack("<d", x) for x in pa.values()] == [struct.pack("<d", x) for x in pb.values()], g
            assert struct.pack("<d", za) == struct.pack("<d", zb), g
