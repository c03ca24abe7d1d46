"""CPU checks of the playout cap's host side: the NumPy plan (engine.playout_plan) and the host model the GPU tests compare
the engine with (tests/playout_cap_model.py), held to oracle.self_play_game where the cap is one in name only."""
import struct

import numpy as np
import pytest

from chinesechessai_amd.engine import normalise_playout_cap, playout_cap_threshold, playout_plan
from oracle import xq_oracle as xo
from tests import playout_cap_model as pm

SEEDS = list(range(7000, 7064))


@pytest.fixture(scope="module")
def uniforms():
    return np.stack([pm.game_uniforms(s) for s in SEEDS])                  # [64][70]


def _mix64_int(x):
    m = (1 << 64) - 1
    x ^= x >> 30; x = (x * 0xbf58476d1ce4e5b9) & m
    x ^= x >> 27; x = (x * 0x94d049bb133111eb) & m
    return x ^ (x >> 31)


def test_plan_is_the_documented_hash(uniforms):
    """h = mix64(seed ^ mix64(bits of the double)); full iff (h >> 40) < round(p * 2^24) - in Python integers"""
    for seed, p in ((0, 0.25), (12345, 0.5), (2 ** 64 - 1, 0.3)):
        got = playout_plan(uniforms[:3], seed, p)
        for g in range(3):
            for ply in range(70):
                bits = struct.unpack("<Q", struct.pack("<d", float(uniforms[g, ply])))[0]
                h = _mix64_int(seed ^ _mix64_int(bits))
                assert bool(got[g, ply]) == ((h >> 40) < int(np.floor(p * 2 ** 24 + 0.5))), (seed, p, g, ply)
    assert playout_cap_threshold(1.0) == 2 ** 24 and playout_cap_threshold(0.25) == 2 ** 22


def test_a_games_plan_does_not_depend_on_its_neighbours(uniforms):
    whole = playout_plan(uniforms, 12345, 0.25)
    for g in (0, 17, 63):
        assert np.array_equal(playout_plan(uniforms[g], 12345, 0.25), whole[g])
    perm = np.random.RandomState(1).permutation(len(SEEDS))
    assert np.array_equal(playout_plan(uniforms[perm], 12345, 0.25), whole[perm])


def test_share_of_full_plies(uniforms):
    """the one statistical statement: over 64 games x 70 plies the full share lies within 4 sqrt(p (1 - p) / n) of p"""
    n = uniforms.size
    for seed in (0, 1, 12345):
        for p in (0.25, 0.5):
            share = playout_plan(uniforms, seed, p).mean()
            bound = 4 * np.sqrt(p * (1 - p) / n)
            print("seed %d p %.2f: share %.4f, |share - p| %.4f, bound %.4f" % (seed, p, share, abs(share - p), bound))
            assert abs(share - p) <= bound, (seed, p, share)


def test_full_prob_one_is_all_full(uniforms):
    for seed in (0, 1, 12345):
        assert playout_plan(uniforms, seed, 1.0).all()


def test_playout_cap_argument_forms():
    assert normalise_playout_cap(None) is None
    want = {"full_prob": 0.25, "fast_sims": 16, "seed": 0, "record_fast": False}
    assert normalise_playout_cap((0.25, 16)) == want
    assert normalise_playout_cap({"full_prob": 0.25, "fast_sims": 16}) == want
    assert normalise_playout_cap({"full_prob": 0.5, "fast_sims": 9, "seed": 7, "record_fast": True}) == {
        "full_prob": 0.5, "fast_sims": 9, "seed": 7, "record_fast": True}
    for bad in (0.25, (0.25,), {"full_prob": 0.25}, {"full_prob": 0.25, "fast_sims": 16, "sims": 50}):
        with pytest.raises(ValueError):
            normalise_playout_cap(bad)


def test_cap_with_an_opponent_is_refused_before_any_device_call(monkeypatch):
    from chinesechessai_amd import self_play as sp
    from chinesechessai_amd.engine import HashNetEvaluator

    def boom(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(sp, "SelfPlayEngine", boom)
    with pytest.raises(ValueError, match="playout_cap"):
        sp.self_play_epoch(HashNetEvaluator(0), 4, 1.0, 50, opponent_network=HashNetEvaluator(1), playout_cap=(0.25, 16))
    with pytest.raises(ValueError, match="playout_cap"):
        sp.parallel_self_play(HashNetEvaluator(0), 4, 1.0, 50, opponent_network=HashNetEvaluator(1), playout_cap=(0.25, 16))


def _same_as_oracle(g, og):
    assert og.error == 0 and g.error == 0
    assert (g.n_plies, g.n_samples, g.winner, g.reason, g.reason_side, g.reason_count) == (
        og.n_plies, og.n_samples, og.winner, og.end_reason, og.end_side, og.end_count)
    for i in range(og.n_plies):
        assert g.chosen[i] == og.t_move[i], i
    for i in range(og.n_samples):
        n = og.s_nmoves[i]
        assert g.moves[i] == list(og.s_moves[i][:n]) and g.counts[i] == list(og.t_visits[i][:n]), i
        assert g.pi[i].tobytes() == np.array(og.s_probs[i][:n], np.float64).tobytes(), i
        assert struct.pack("<d", g.z[i]) == struct.pack("<d", og.s_z[i]), i
        assert g.players[i] == og.s_player[i] and bytes(g.boards[i].tobytes()) == bytes(og.s_board[i]), i


@pytest.mark.parametrize("form", ("full_prob_1", "fast_equals_sims"))
def test_model_equals_the_oracle_where_the_cap_changes_nothing(form):
    """seeds 7000..7015 at 50 simulations: moves, counts, pi, z, winner and reason of the model's games equal
    oracle.self_play_game's"""
    S = 50
    for seed in SEEDS[:16]:
        rc, og = xo.self_play_game(seed, S)
        assert rc == 0
        g = pm.play(seed, S, 1.0, 16, cap_seed=5) if form == "full_prob_1" else pm.play(seed, S, 0.25, S, cap_seed=5)
        assert all(b == S for b in g.sims)
        _same_as_oracle(g, og)


def test_z_table_of_a_capped_game_counts_every_ply():
    """a capped game's z table is self_play.py:259-310 over ALL its stored plies: the length thresholds (30 / 50 / 60 / 70)
    see n_samples, not the number of full plies - and the model's restatement of the table is the oracle's xqo_z_value"""
    L = xo.lib()
    for winner in (-1, 0, 1):
        for player in (-1, 1):
            for length in (1, 29, 30, 31, 50, 51, 59, 60, 61, 70):
                for reward in (None, 0.0, 0.37, -1.5):
                    want = L.xqo_z_value(winner, player, length, 0 if reward is None else 1, 0.0 if reward is None else reward)
                    assert struct.pack("<d", pm.z_value(winner, player, length, reward)) == struct.pack("<d", want)
    seen_fast = 0
    for seed in SEEDS[:6]:
        g = pm.play(seed, 50, 0.25, 16, cap_seed=12345)
        n_full = sum(g.full)
        assert g.n_samples == g.n_plies == len(g.z) and 0 < n_full < g.n_samples
        seen_fast += g.n_samples - n_full
        assert [b for b in g.sims] == [50 if f else 16 for f in g.full]
        assert [sum(c) for c in g.counts] == [b - 8 for b in g.sims]         # the first 8 simulations land on the root
        for i in range(g.n_samples):
            r = g.rewards[i] if i < g.n_plies else None
            assert g.z[i] == pm.z_value(g.winner, g.players[i], g.n_samples, r)
            if g.n_samples != n_full and (g.n_samples >= 60) != (n_full >= 60) and g.winner == 0:
                assert g.z[i] != pm.z_value(g.winner, g.players[i], n_full, r)   # (a table over full plies only would differ)
    assert seen_fast > 0
