"""Last round visits only (xq_engine_set_last_round_visits_only), the argument on the CPU: what the evaluator says about
the leaf of a ply's LAST search round reaches no root visit count.  No GPU.

tests/search_mirror.py is imported unchanged.  Its search cannot be told from outside to park nothing in its last round
(the pending list is local to search_mirror), so `search_visits_only` below restates the mirror's loop - with the mirror's
own Node, _select and _backup - and changes the one thing the engine changes: in the last round of a search of more than
one round, a non-terminal leaf is not evaluated, not expanded and not backed up; the round's remaining simulations are
booked as visits along its path.  A second check needs no restatement: the mirror itself, handed garbage for exactly
those leaves, must not notice."""
import zlib

import numpy as np
import pytest

from oracle import xq_oracle as xo

from tests import search_mirror as sm


def seeded_evaluator(seed):
    """random priors (float32, normalised) and a random value in (-1, 1), keyed by the position and `seed`"""
    def evaluate(board90, player, legal):
        h = zlib.crc32(np.asarray(board90, dtype=np.int8).reshape(90).tobytes() + bytes([int(player) & 0xff, seed & 0xff]))
        rng = np.random.RandomState(h)
        p = rng.random_sample(len(legal)).astype(np.float32) + np.float32(1e-3)
        p = p / p.sum(dtype=np.float32)
        return [np.float32(x) for x in p], float(rng.uniform(-1, 1))
    return evaluate


def search_visits_only(game_env, sims, leaf_batch, evaluate):
    """search_mirror's loop (fresh root, no virtual loss) with the last round booking visits only.  Returns (root moves,
    root child visits, root, number of leaves evaluated)."""
    L = xo.lib()
    root, arena = sm.Node(), [1]
    env = xo.OracleEnv()
    pending = []
    rounds = (sims + leaf_batch - 1) // leaf_batch
    evaluated = 0

    def consume():
        for node, path, mult, moves, pri, val in pending:
            node.ch = [sm.Node(p, m, arena[0] + j) for j, (p, m) in enumerate(zip(pri, moves))]
            arena[0] += len(moves)
            sm._backup(root, path, val, mult)
        pending.clear()

    done, rnd = 0, 0
    while done < sims:
        batch = min(leaf_batch, sims - done)
        last = rnd == rounds - 1 and rounds > 1
        consume()
        left = batch
        while left > 0:
            node, path = root, []
            while node.ch:
                node = sm._select(node)
                path.append(node)
            if not node.term:
                L.xqo_copy_min(env.p, game_env.p)
                for x in path:
                    env.make_move(x.mv)
                legal = env.legal_moves()
                w = int(env.e.winner)
                side = int(env.e.current_player)
                if legal and w == xo.WINNER_NONE:
                    if last and node is not root:
                        for x in [root] + path:              # visits only: no evaluation, no expansion, no value
                            x.N += left
                        break
                    pri, val = evaluate(env.board().reshape(90), side, legal)
                    evaluated += 1
                    pending.append([node, list(path), left, legal, pri, val])
                    break
                node.term = True
                node.val = 1.0 if w == side else (-1.0 if w == -side else 0.0)
            sm._backup(root, path, node.val, 1)
            left -= 1
        done += batch
        rnd += 1
    consume()
    return [c.mv for c in root.ch], [c.N for c in root.ch], root, evaluated


@pytest.fixture(scope="module")
def positions():
    envs, _ = sm.seeded_positions(seed=20261126, count=10, step=4)
    assert len(envs) >= 6
    return envs


@pytest.mark.parametrize("sims", [15, 16, 50, 23])
def test_visits_only_last_round_gives_the_mirrors_root_visits(positions, sims):
    """sims 15 (last round of 7), 16 (of 8), 50 (7 rounds, last of 2), 23 (3 rounds): the same root moves and root visits,
    the same visit count on every node both trees hold, one evaluation fewer unless the last round met a terminal leaf."""
    for seed in (1, 2, 3):
        ev = seeded_evaluator(seed)
        for env in positions:
            calls = [0]

            def counting(b, p, legal, ev=ev, calls=calls):
                calls[0] += 1
                return ev(b, p, legal)
            moves, visits, root = sm.search_mirror(env, sm.Node(), sims, 8, False, counting)
            moves2, visits2, root2, evaluated = search_visits_only(env, sims, 8, ev)
            assert moves == moves2 and visits == visits2
            assert sum(visits) == sims - 8 and root.N == root2.N == sims
            assert evaluated in (calls[0], calls[0] - 1)
            # node by node: the visits-only tree is the mirror's tree without the last leaf's children
            stack = [(root, root2)]
            unexpanded = 0
            while stack:
                x, y = stack.pop()
                assert x.N == y.N and x.mv == y.mv
                if x.ch and not y.ch:
                    unexpanded += 1
                    assert all(c.N == 0 for c in x.ch)           # the mirror's last leaf: children nobody visited
                    continue
                assert len(x.ch) == len(y.ch)
                stack.extend(zip(x.ch, y.ch))
            assert unexpanded == calls[0] - evaluated


def test_one_round_search_is_left_alone(positions):
    """sims <= leaf_batch: the only round parks the root, visits-only or not (root visits stay empty: the NaN error path)"""
    ev = seeded_evaluator(5)
    for sims in (5, 8):
        moves, visits, root = sm.search_mirror(positions[0], sm.Node(), sims, 8, False, ev)
        moves2, visits2, root2, evaluated = search_visits_only(positions[0], sims, 8, ev)
        assert moves == moves2 and visits == visits2 == [0] * len(moves) and evaluated == 1
        assert root.N == root2.N == sims and root.W == root2.W


def test_the_mirror_itself_ignores_the_last_rounds_evaluation(positions):
    """No restatement here: search_mirror with an evaluator that answers garbage - other priors, another value - for
    whatever it is asked in the last round returns the same root visits."""
    for sims in (15, 50):
        rounds = (sims + 7) // 8
        for env in positions:
            ev = seeded_evaluator(7)
            asked = []

            def honest(b, p, legal):
                asked.append(1)
                return ev(b, p, legal)
            ref = sm.search_mirror(env, sm.Node(), sims, 8, False, honest)[:2]
            n_honest = len(asked)
            garbage = seeded_evaluator(99)
            seen = []

            def lying(b, p, legal):
                seen.append(1)
                # (evaluations are asked one per round unless a round ends on terminal leaves: the last one asked is the
                # last round's exactly when every round asked)
                if len(seen) == rounds and n_honest == rounds:
                    pri, val = garbage(b, p, legal)
                    return pri, -val
                return ev(b, p, legal)
            got = sm.search_mirror(env, sm.Node(), sims, 8, False, lying)[:2]
            assert got == ref
