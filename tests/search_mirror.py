"""Test-side restatement of the engine's search, one evaluator shared by the engine and the oracle.

TEST INFRASTRUCTURE ONLY (not a test module, not a conftest).  Five things live here:

  peaked_eval         a deterministic "trained network" stand-in: almost all prior mass on one legal move chosen by
                      CRC-32 of the position, a small dyadic value.  Wrapped once as an oracle callback
                      (peaked_oracle_evaluator) and once as a predict_batch object (PeakedNet, for
                      engine.CallbackEvaluator), so the GPU engine and the CPU oracle read identical fp32 priors and
                      fp64 values.  Peaked priors make the search follow one line: 64 rounds reach level 63, and a
                      reused tree grows past level 64 within three plies.
  uniform_*           all priors float32(1) / float32(n), value 0, behind the same three wrappers: every unvisited child
                      ties, only first-index order decides (tests/test_wide_nodes_cpu.py, tests/test_gpu_wide_nodes.py).
  search_mirror       Python restatement of one MCTS.search (self_play.py:89-154) as the engine runs it: NumPy float32
                      stepwise PUCT, ordered float64 backup, one pending leaf per round of `leaf_batch` simulations - or,
                      with virtual_loss, up to `leaf_batch` pending leaves, a pending visit counting as N + 1, W - 1 on
                      every node of its path.  It starts from a given game env and a given Node: a fresh one, or the
                      subtree kept from the previous ply (the engine's opt-in tree reuse).
  play_reuse_mirror   from the start position or a given env; per ply: search, record the tree, play the argmax child,
                      keep its subtree if it was expanded (k_play_move), otherwise start fresh.

tests/test_search_mirror_cpu.py validates the mirror against the pinned oracle's search_tree before any GPU test trusts it.
"""
import ctypes as C
import zlib

import numpy as np

from oracle import xq_oracle as xo

PEAK = 0.97


class Node:
    """idx = the node's index in creation order, which is its index in the engine's per-game arena (0 = a fresh root)"""
    __slots__ = ("N", "W", "P", "mv", "ch", "term", "val", "vl", "idx")

    def __init__(self, P=np.float32(0), mv=0, idx=0):
        self.N, self.W, self.P, self.mv, self.ch, self.term, self.val, self.vl = 0, 0.0, P, mv, [], False, 0.0, 0
        self.idx = idx


# ---- evaluators --------------------------------------------------------------------------------------------------------
def peaked_eval(board90, player, n_moves):
    """(index of the move that gets the peak, value) for a position: keyed by crc32(90 board bytes + side byte)."""
    h = zlib.crc32(np.asarray(board90, dtype=np.int8).reshape(90).tobytes() + bytes([int(player) & 0xff]))
    return h % n_moves, ((h >> 4) % 5 - 2) / 256


def peaked_priors(n_moves, peak_index, peak=PEAK):
    """the fp32 priors both sides read: `peak` on one move, the rest shared evenly"""
    rest = np.float32((1 - peak) / (n_moves - 1)) if n_moves > 1 else np.float32(0)
    p = np.full(n_moves, rest, dtype=np.float32)
    p[peak_index] = np.float32(peak)
    return p


def peaked_evaluate(board90, player, legal):
    """search_mirror's evaluator interface: (list of np.float32 priors in legal-move order, float value)"""
    idx, val = peaked_eval(board90, player, len(legal))
    return list(peaked_priors(len(legal), idx)), val


def hashnet_evaluate(board90, player, legal):
    """the oracle's HashNet behind the same interface"""
    h0 = zlib.crc32(np.asarray(board90, dtype=np.int8).reshape(90).tobytes() + bytes([int(player) & 0xff]))
    pri = []
    for mv in legal:
        f, t = divmod(int(mv), 90)
        h = zlib.crc32(bytes([f // 9, f % 9, t // 9, t % 9]), h0)
        pri.append(np.float32(((h >> 8) % 64 + 1) / 1024))
    return pri, ((h0 >> 4) % 65 - 32) / 64


def peaked_oracle_evaluator():
    """xo.Evaluator whose callback is peaked_eval (the returned object keeps the callback alive)"""
    def fn(ctx, nrows, boards, players, moves, nmoves, priors, values):
        for i in range(nrows):
            n = int(nmoves[i])
            b = np.ctypeslib.as_array(boards, shape=((i + 1) * 90,))[i * 90:(i + 1) * 90]
            idx, val = peaked_eval(b, int(players[i]), n)
            p = peaked_priors(n, idx)
            for j in range(n):
                priors[i * xo.MAX_MOVES + j] = p[j]
            values[i] = val
        return 0
    cb = xo.EVAL_FN(fn)
    ev = xo.Evaluator(cb, None)
    ev._keep = cb
    return ev


class PeakedNet:
    """reference-style network object for engine.CallbackEvaluator: predict_batch([(board, player, legal)])"""

    def predict_batch(self, rows):
        out = []
        for board, player, legal in rows:
            idx, val = peaked_eval(np.asarray(board, dtype=np.int8).reshape(90), player, len(legal))
            p = peaked_priors(len(legal), idx)
            out.append(({mv: p[j] for j, mv in enumerate(legal)}, val))
        return out


def uniform_priors(n_moves):
    """all priors float32(1) / float32(n): every unvisited child ties, only first-index order decides"""
    return np.full(n_moves, np.float32(1) / np.float32(n_moves), dtype=np.float32)


def uniform_evaluate(board90, player, legal):
    """search_mirror's evaluator interface for the uniform evaluator (value 0)"""
    return list(uniform_priors(len(legal))), 0.0


def uniform_oracle_evaluator():
    """xo.Evaluator handing out uniform_priors and value 0"""
    def fn(ctx, nrows, boards, players, moves, nmoves, priors, values):
        for i in range(nrows):
            n = int(nmoves[i])
            p = uniform_priors(n)
            for j in range(n):
                priors[i * xo.MAX_MOVES + j] = p[j]
            values[i] = 0.0
        return 0
    cb = xo.EVAL_FN(fn)
    ev = xo.Evaluator(cb, None)
    ev._keep = cb
    return ev


class UniformNet:
    """predict_batch object of the uniform evaluator for engine.CallbackEvaluator"""

    def predict_batch(self, rows):
        out = []
        for board, player, legal in rows:
            p = uniform_priors(len(legal))
            out.append(({mv: p[j] for j, mv in enumerate(legal)}, 0.0))
        return out


# ---- the search --------------------------------------------------------------------------------------------------------
def _select(node):
    """self_play.py:40-59 under NumPy >= 2: every step rounded to float32, the first maximum wins"""
    sq = np.float32(np.sqrt(np.float64(node.N + node.vl)))
    best, bi = None, -1
    for i, c in enumerate(node.ch):
        n, w = c.N + c.vl, c.W - float(c.vl)
        q = np.float32(w / n) if n else np.float32(0)
        t = np.float32(1.5) * c.P
        t = t * sq
        t = t / np.float32(1 + n)
        sc = q + t
        if best is None or sc > best:
            best, bi = sc, i
    return node.ch[bi]


def _backup(root, path, v, mult):
    """self_play.py:70-80: `mult` sequential float64 updates at the leaf, the sign alternating towards the root"""
    depth = len(path)
    for lvl in range(depth + 1):
        x = root if lvl == 0 else path[lvl - 1]
        sv = -v if ((depth - lvl) & 1) else v
        for _ in range(mult):
            x.W += sv
        x.N += mult


def search_mirror(game_env, root, sims, leaf_batch=8, virtual_loss=False, evaluate=peaked_evaluate, arena=None):
    """One search of `sims` simulations below `root` (a fresh Node, or a kept subtree) for the position in `game_env`
    (an xo.OracleEnv; it is not changed).  Every simulation replays its path on a copy of the game env with an empty
    position history (_copy_env, self_play.py:156-175).  A node classified terminal stays terminal with its value (the
    engine keeps that in the node's flags).  `arena`: one-element list holding the number of nodes created so far (a kept
    subtree goes on numbering where the last ply stopped, like the engine's arena).  Returns (root moves, root child
    visits, root)."""
    L = xo.lib()
    if arena is None:
        arena = [1]
    env = xo.OracleEnv()
    pending = []

    def consume():
        for node, path, mult, moves, pri, val in pending:
            node.ch = [Node(p, m, arena[0] + j) for j, (p, m) in enumerate(zip(pri, moves))]
            arena[0] += len(moves)
            if virtual_loss:
                for x in [root] + path:
                    x.vl -= mult
            _backup(root, path, val, mult)
        pending.clear()

    done = 0
    while done < sims:
        batch = min(leaf_batch, sims - done)
        consume()
        left = batch
        while left > 0:
            node, path = root, []
            while node.ch:
                node = _select(node)
                path.append(node)
            if virtual_loss and not node.term and node.vl:
                # already waiting for the evaluator in this round: one more pending visit through the same path
                for e in pending:
                    if e[0] is node:
                        e[2] += 1
                for x in [root] + path:
                    x.vl += 1
                left -= 1
                continue
            if not node.term:
                L.xqo_copy_min(env.p, game_env.p)
                for x in path:
                    env.make_move(x.mv)
                legal = env.legal_moves()
                w = int(env.e.winner)
                side = int(env.e.current_player)
                if legal and w == xo.WINNER_NONE:
                    pri, val = evaluate(env.board().reshape(90), side, legal)
                    if virtual_loss:
                        pending.append([node, list(path), 1, legal, pri, val])
                        for x in [root] + path:
                            x.vl += 1
                        left -= 1
                        continue
                    # the tree is frozen until the evaluator answers: the round's remaining simulations reach this leaf too
                    pending.append([node, list(path), left, legal, pri, val])
                    break
                node.term = True
                node.val = 1.0 if w == side else (-1.0 if w == -side else 0.0)
            _backup(root, path, node.val, 1)
            left -= 1
        done += batch
    consume()
    assert root.vl == 0
    return [c.mv for c in root.ch], [c.N for c in root.ch], root


def play_reuse_mirror(sims, plies, start_moves=(), leaf_batch=8, virtual_loss=False, evaluate=peaked_evaluate, reuse=True,
                      start_env=None):
    """`plies` plies of argmax play from the start position after `start_moves` - or from a copy of the xo.OracleEnv
    `start_env` (any position, e.g. one made with set_state; it is not changed) after `start_moves` -, each searched with
    search_mirror; with `reuse` the played child's subtree is the next ply's tree if it was expanded (k_play_move),
    otherwise the tree is fresh.  Returns a list per ply of dict(flat=flatten_nodes of the tree as searched - a snapshot:
    a kept subtree goes on changing -, root_idx, moves, counts, played)."""
    env = xo.OracleEnv()
    if start_env is None:
        env.reset()
    else:
        C.memmove(env.p, start_env.p, C.sizeof(xo.Env))
    for m in start_moves:
        env.make_move(int(m))
    root, out, arena = Node(), [], [1]
    for _ in range(plies):
        moves, counts, root = search_mirror(env, root, sims, leaf_batch, virtual_loss, evaluate, arena)
        am = int(np.argmax(np.asarray(counts)))                 # the first maximum (self_play.py:224-227)
        out.append(dict(flat=flatten_nodes(root), root_idx=root.idx, moves=moves, counts=counts, played=moves[am]))
        env.make_move(moves[am])
        child = root.ch[am]
        if reuse and child.ch:
            root = child
        else:
            root, arena = Node(), [1]
    return out


# ---- views of a mirror tree --------------------------------------------------------------------------------------------
def flatten_nodes(root):
    """The tree below `root` walked in child order: per node (depth, move, N, W bits, P bits, child count, index of the
    first child or -1)."""
    out = []
    stack = [(root, 0)]
    while stack:
        node, d = stack.pop()
        out.append((d, int(node.mv), int(node.N), np.float64(node.W).view(np.uint64).item(),
                    np.float32(node.P).view(np.uint32).item(), len(node.ch), node.ch[0].idx if node.ch else -1))
        for c in reversed(node.ch):
            stack.append((c, d + 1))
    return out


def flatten_arrays(tree, root_index=0):
    """the same child-order walk over a tree given as arrays (oracle search_tree / engine read_tree)"""
    out = []
    N, W, P = tree["visit_count"], tree["value_sum"], tree["prior"]
    mv, fc, nc = tree["move"], tree["first_child"], tree["n_child"]
    Wb, Pb = np.ascontiguousarray(W, np.float64).view(np.uint64), np.ascontiguousarray(P, np.float32).view(np.uint32)
    stack = [(int(root_index), 0)]
    while stack:
        i, d = stack.pop()
        k = int(nc[i])
        f = int(fc[i])
        out.append((d, int(mv[i]), int(N[i]), int(Wb[i]), int(Pb[i]), k, f if k else -1))
        for j in range(k - 1, -1, -1):
            stack.append((f + j, d + 1))
    return out


def visited_depths(flat):
    """depths of the nodes with at least one visit, from a flatten_* list"""
    return [t[0] for t in flat if t[2] > 0]


# ---- positions ---------------------------------------------------------------------------------------------------------
def seeded_positions(seed=20261005, count=12, step=3):
    """Oracle envs reached by seeded random play, position k after step * k plies (the construction of
    test_search_tree_equals_oracle_node_by_node); lines that end early are left out.  Returns (envs, lines)."""
    rng = np.random.RandomState(seed)
    envs, lines = [], []
    for k in range(count):
        oe = xo.OracleEnv()
        oe.reset()
        line = []
        for _ in range(step * k):
            mv = oe.legal_moves()
            if not mv or oe.e.winner != xo.WINNER_NONE:
                break
            m = int(mv[rng.randint(len(mv))])
            line.append(m)
            oe.make_move(m)
        if oe.e.winner == xo.WINNER_NONE and oe.legal_moves():
            envs.append(oe)
            lines.append(line)
    return envs, lines
