"""Host model of one playout-capped self-play game (xq_engine_set_playout_cap), driven over the CPU oracle's public API.

Per ply: (1) the plan - full or fast - from the game's own MT19937 doubles (engine.playout_plan), (2) OracleEnv.search with
that ply's budget and the HashNet evaluator, (3) pi as distributed.record_to_sample forms it from the visit counts,
(4) xqo_choice_from_uniform on the ply's double, (5) make_move; at the end (6) the z table of self_play.py:259-310,
restated here in Python over ALL stored plies: a fast ply is a sample like any other, so the table's length thresholds
do not move.  With full_prob = 1 or fast_sims = sims the model is oracle.self_play_game (tests/test_playout_cap_cpu.py
holds it to that before a GPU sees it).

TEST INFRASTRUCTURE ONLY (it imports the oracle)."""
import ctypes as C

import numpy as np

from chinesechessai_amd.engine import playout_plan
from oracle import xq_oracle as xo

MAX_PLIES = 70
MAX_MOVES = 128


def game_uniforms(seed):
    """the 70 doubles np.random.choice consumes in the game seeded with `seed` (np.random.seed(seed), one per ply)"""
    return np.random.RandomState(int(seed)).random_sample(MAX_PLIES)


def z_value(winner, player, length, reward):
    """self_play.py:266-310 for one sample (`reward` None: no step reward for that index)"""
    if winner == 0:
        fr = (-0.15 if player == 1 else 0.05) if length >= 60 else (-0.1 if player == 1 else 0.1)
    elif winner == player:
        fr = 1.0 + (0.5 if length <= 30 else 0.3 if length <= 50 else 0.1 if length <= 70 else 0.0)
    else:
        fr = -1.2 if length >= 60 else -1.0
    imm = 0.0 if reward is None else reward
    return fr + imm * 0.01


def pi_of_counts(counts, temperature=1.0):
    """distributed.record_to_sample's move probabilities"""
    c = np.asarray(counts, dtype=np.int64)
    if temperature < 0.01:
        p = np.zeros(len(c))
        p[np.argmax(c)] = 1
        return p
    c = c ** (1.0 / temperature)
    return c / c.sum()


class ModelGame:
    """what the engine is compared with, field by field"""

    def __init__(self):
        self.moves, self.counts, self.pi, self.boards, self.players = [], [], [], [], []
        self.chosen, self.rewards, self.sims, self.full = [], [], [], []
        self.z = []
        self.winner = self.reason = self.reason_side = self.reason_count = 0
        self.n_plies = self.n_samples = 0
        self.error = 0


def play(seed, sims, full_prob, fast_sims, cap_seed=0, max_moves=70, env=None, uniforms=None):
    """One capped game.  fast_sims = 0: no cap (every ply full).  `env`: start from this OracleEnv (else the start
    position); `uniforms`: override the game's doubles."""
    L = xo.lib()
    u = game_uniforms(seed) if uniforms is None else np.asarray(uniforms, dtype=np.float64)
    full = playout_plan(u, cap_seed, full_prob) if fast_sims else np.ones(MAX_PLIES, bool)
    oe = env if env is not None else xo.OracleEnv()
    ev = xo.hashnet_evaluator()
    g = ModelGame()
    for ply in range(min(max_moves, MAX_PLIES)):
        player = int(oe.e.current_player)
        if not oe.legal_moves():                                   # self_play.py:205-208
            break
        budget = sims if full[ply] else fast_sims
        moves, visits = oe.search(budget, ev)                      # self_play.py:214
        if not moves:                                              # :216-217
            break
        p = np.ascontiguousarray(pi_of_counts(visits), dtype=np.float64)
        g.boards.append(oe.board().reshape(90))
        g.players.append(player)
        g.moves.append(moves)
        g.counts.append(visits)
        g.pi.append(p)
        g.sims.append(budget)
        g.full.append(bool(full[ply]))
        idx = L.xqo_choice_from_uniform(p.ctypes.data_as(C.POINTER(C.c_double)), len(moves), float(u[ply]))   # :242
        if idx < 0:
            g.error = 1
            break
        idx = min(idx, len(moves) - 1)
        g.chosen.append(moves[idx])
        reward, done, _ = oe.make_move(moves[idx])                 # :246
        g.rewards.append(reward)
        if done:
            break
    e = oe.e
    g.winner = 0 if e.winner == xo.WINNER_NONE else int(e.winner)  # :259
    g.reason, g.reason_side, g.reason_count = int(e.end_reason), int(e.end_side), int(e.end_count)
    g.n_plies, g.n_samples = len(g.chosen), len(g.moves)
    g.z = [z_value(g.winner, g.players[i], g.n_samples, g.rewards[i] if i < g.n_plies else None)
           for i in range(g.n_samples)]
    return g
