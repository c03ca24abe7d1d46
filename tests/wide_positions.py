"""Positions whose side to move has 64 legal moves or more (TEST INFRASTRUCTURE ONLY: not a test module).

One wavefront plays one game; from 65 legal moves on, lane l also carries child l + 64.  No opening position, no fixture and
no self-play game of the suite reaches that width, so the boards below are what tests/test_wide_nodes_cpu.py and
tests/test_gpu_wide_nodes.py search.  They were found once by a seeded hill-climb on the CPU against the rules oracle (random
placement on lawful squares, one piece moved per step, the oracle's legal-move count as the score) and are committed as
literal placements, in the style of edge_boards() of oracle/gen_golden.py; `many_moves` is that function's board.

Every board: kings in their palaces with true king caches; advisors, bishops and pawns on squares they can lawfully occupy
(so every legal move has a column in the reachable-column map); the side to move is not in check (nor is the other side,
except the bare black king of `many_moves`); no pseudo-legal move of the side to move is suicidal, so the pseudo-legal
count equals the width and stays within the 128 candidates the device's move generator keeps before its suicide filter
(xq_selfplay.h, xq_rules_legal_moves).  tests/test_wide_nodes_cpu.py asserts all of
it, and that bound for every node the searches of the tests expand."""
import ctypes as C

import numpy as np

from oracle import xq_oracle as xo
from tests import search_mirror as sm

K, A, B, N, R, Cn, Pw = 1, 2, 3, 4, 5, 6, 7

# (name, width = legal moves of the side to move, width of the other side were it to move, {square: piece}, side to move,
#  red king, black king)
BOARDS = [
    ("w64", 64, 21,
     {(0, 2): -B, (0, 3): -K, (1, 2): N, (1, 3): Pw, (2, 0): -N, (2, 3): -A, (3, 1): Pw, (3, 5): Cn, (4, 6): Pw, (5, 2): R,
      (5, 3): N, (5, 6): -R, (6, 4): Cn, (6, 8): -Pw, (7, 0): -Pw, (7, 3): K, (7, 4): B, (7, 5): R, (8, 4): A},
     1, (7, 3), (0, 3)),
    ("w65", 65, 18,
     {(0, 3): -A, (0, 4): Pw, (1, 2): -N, (1, 5): -K, (2, 0): -B, (2, 4): -B, (2, 7): Cn, (2, 8): Pw, (3, 5): N, (4, 0): -Pw,
      (4, 6): Cn, (4, 8): -Pw, (5, 2): R, (6, 7): R, (7, 3): K, (7, 5): A, (8, 4): A, (8, 6): -Cn, (9, 2): B},
     1, (7, 3), (1, 5)),
    # the material of the start position on both sides, both sides wide (the roots of the next two plies of argmax play too)
    ("lawful_both", 71, 70,
     {(0, 2): -B, (0, 3): -A, (0, 4): -K, (0, 5): -A, (0, 6): -B, (0, 8): Pw, (1, 0): Pw, (1, 2): Pw, (1, 5): Cn, (1, 6): -N,
      (1, 8): -R, (2, 2): Pw, (2, 4): -R, (2, 7): R, (3, 1): -Cn, (4, 0): -Pw, (4, 2): -Pw, (4, 3): R, (5, 0): Pw, (5, 2): B,
      (5, 6): -Cn, (6, 4): N, (7, 0): -N, (7, 2): -Pw, (7, 3): Cn, (8, 3): K, (8, 4): -Pw, (8, 6): N, (9, 3): A, (9, 5): A,
      (9, 6): B, (9, 8): -Pw},
     1, (8, 3), (0, 4)),
    # the same material, black to move
    ("lawful_both_black", 71, 69,
     {(0, 2): -B, (0, 3): -A, (0, 4): Pw, (0, 5): -K, (1, 0): -Cn, (1, 6): R, (1, 8): Pw, (2, 3): -A, (2, 4): -B, (2, 8): Pw,
      (3, 1): -R, (3, 6): -R, (3, 8): Pw, (4, 0): -Cn, (4, 7): Cn, (5, 4): -N, (5, 6): B, (5, 8): -Pw, (6, 2): Cn, (6, 8): Pw,
      (7, 1): R, (7, 5): N, (8, 3): -Pw, (8, 4): K, (8, 5): -Pw, (8, 7): -N, (9, 0): -Pw, (9, 1): N, (9, 2): B, (9, 3): A,
      (9, 5): A, (9, 7): -Pw},
     -1, (8, 4), (0, 5)),
    # edge_boards()'s `many_moves` (tests/golden/rules_edge.json)
    ("many_moves", 72, 0,
     {(4, 4): R, (5, 3): R, (4, 1): Cn, (6, 6): Cn, (5, 5): N, (3, 2): N, (9, 4): K, (0, 3): -K, (6, 0): Pw, (4, 8): Pw,
      (3, 6): Pw},
     1, (9, 4), (0, 3)),
    ("heavy_both", 89, 89,
     {(0, 0): Cn, (0, 3): -K, (0, 5): -A, (0, 6): Pw, (0, 8): N, (1, 4): -Cn, (2, 3): -R, (2, 8): -N, (3, 5): R, (4, 1): R,
      (4, 8): -Cn, (5, 4): R, (5, 7): -R, (6, 1): -N, (6, 6): R, (6, 8): N, (7, 4): Cn, (8, 4): A, (8, 5): K, (8, 8): -Pw,
      (9, 0): -R, (9, 2): -R},
     1, (8, 5), (0, 3)),
    ("w104", 104, 11,
     {(0, 3): -A, (1, 2): R, (1, 3): Pw, (1, 6): Cn, (2, 2): R, (2, 4): -B, (2, 5): -K, (2, 7): Pw, (3, 2): N, (3, 5): N,
      (4, 8): Cn, (5, 6): R, (6, 0): R, (7, 0): -Pw, (7, 1): R, (7, 4): B, (8, 3): K, (8, 4): A, (8, 7): -Pw, (9, 0): Cn,
      (9, 6): -N},
     1, (8, 3), (2, 5)),
    ("w128", 128, 6,
     {(0, 3): -A, (0, 5): -K, (1, 0): Pw, (1, 2): N, (1, 7): R, (2, 3): R, (2, 5): Cn, (3, 0): Pw, (3, 8): R, (4, 2): R,
      (4, 6): -B, (5, 0): Cn, (6, 2): R, (7, 2): N, (7, 4): B, (8, 1): R, (8, 3): K, (8, 4): A, (8, 6): -Pw, (9, 2): Cn},
     1, (8, 3), (0, 5)),
]

ALL_NAMES = [b[0] for b in BOARDS]
# `w128` sits on the cap.  Every tree the one-leaf, virtual-loss and two-network tests build from it stays within 128
# pseudo-legal moves per expanded node (tests/test_wide_nodes_cpu.py walks them), so those tests take ALL_NAMES.  Three plies
# of sampled play with the sampler tests' evaluator do not: two plies below the board a line opens and red has more than
# 128 pseudo-legal moves, which neither the device nor the oracle's 128-entry move lists hold.  That plan takes
# SAMPLER_NAMES; `w128` goes through the sampler for one ply of the HashNet tree instead (SAMPLER_ONE_PLY).
SAMPLER_ONE_PLY = ["w128"]
SAMPLER_NAMES = [n for n in ALL_NAMES if n not in SAMPLER_ONE_PLY]
BOTH_WIDE = ["lawful_both", "lawful_both_black", "heavy_both"]      # the other side is wider than 64 too
MAX_CANDIDATES = 128                                                # xq_rules_legal_moves: pseudo-legal moves kept


def entry(name):
    return next(b for b in BOARDS if b[0] == name)


def board90(name):
    b = np.zeros(90, np.int8)
    for (r, c), p in entry(name)[3].items():
        b[r * 9 + c] = p
    return b


def env_of(name, player=None):
    """a fresh xo.OracleEnv holding the board (move_count 0, empty history, true king caches)"""
    _, _, _, _, side, rk, bk = entry(name)
    oe = xo.OracleEnv()
    oe.set_state(board90(name), side if player is None else player, red_king=xo.sq(rk), black_king=xo.sq(bk))
    return oe


def copy_env(oe):
    out = xo.OracleEnv()
    C.memmove(out.p, oe.p, C.sizeof(xo.Env))
    return out


def raw_counts(oe):
    """(legal moves, pseudo-legal moves) of the side to move as the oracle counts them, without the 128-entry limit of
    OracleEnv.legal_moves: with both king caches empty no move is in check or facing, so every pseudo-legal move (on the
    board, not onto an own piece) counts as legal"""
    buf = (C.c_uint16 * xo.MAX_MOVES)()
    n = xo.lib().xqo_legal_moves(oe.p, buf)
    bare = copy_env(oe)
    bare.e.red_king = bare.e.black_king = xo.NO_KING
    return n, xo.lib().xqo_legal_moves(bare.p, buf)


# ---- the three evaluators every tree test uses: name -> (oracle evaluator, mirror evaluate, predict_batch object) --------
def evaluators():
    return {"hashnet": (xo.hashnet_evaluator, sm.hashnet_evaluate, None),
            "peaked": (sm.peaked_oracle_evaluator, sm.peaked_evaluate, sm.PeakedNet),
            "uniform": (sm.uniform_oracle_evaluator, sm.uniform_evaluate, sm.UniformNet)}


# ---- the sampler tests' evaluator: visits on both sides of the 64-child boundary and on the last child ----------------------
def edge_priors(n):
    """0.2 each on children 63, 64 and n - 1 (those that exist), the rest shared evenly; the value is 0: the search visits
    those children and hardly any other, so the sampler's cdf has its steps exactly there"""
    hot = sorted({j for j in (63, 64, n - 1) if 0 <= j < n})
    rest = n - len(hot)
    p = np.full(n, np.float32((1 - 0.2 * len(hot)) / rest) if rest else np.float32(0), dtype=np.float32)
    p[hot] = np.float32(0.2)
    return p


def edge_oracle_evaluator():
    def fn(ctx, nrows, boards, players, moves, nmoves, priors, values):
        for i in range(nrows):
            n = int(nmoves[i])
            p = edge_priors(n)
            for j in range(n):
                priors[i * xo.MAX_MOVES + j] = p[j]
            values[i] = 0.0
        return 0
    cb = xo.EVAL_FN(fn)
    ev = xo.Evaluator(cb, None)
    ev._keep = cb
    return ev


class EdgeNet:
    def predict_batch(self, rows):
        out = []
        for board, player, legal in rows:
            p = edge_priors(len(legal))
            out.append(({mv: p[j] for j, mv in enumerate(legal)}, 0.0))
        return out


_TREES = {}


def oracle_tree(name, sims, evaluator):
    """OracleEnv.search_tree of a board, computed once per process and shared (read-only) by the tests"""
    key = (name, sims, evaluator)
    if key not in _TREES:
        _TREES[key] = env_of(name).search_tree(sims, evaluators()[evaluator][0]())
    return _TREES[key]


_VL_MIRRORS = {}


def vl_mirror(name, sims):
    """root of search_mirror(virtual_loss=True) with the peaked evaluator from a board, computed once per process and shared
    (read-only) by the tests"""
    if (name, sims) not in _VL_MIRRORS:
        _VL_MIRRORS[(name, sims)] = sm.search_mirror(env_of(name), sm.Node(), sims, virtual_loss=True)[2]
    return _VL_MIRRORS[(name, sims)]


def node_envs(start, tree, expanded_only=True):
    """(node index, env at that node) for the nodes of an oracle tree searched from `start` (a board's name or an
    xo.OracleEnv; expanded nodes by default): the moves of the node's path replayed on a copy of the start"""
    parent, move = tree["parent"], tree["move"]
    for i in range(len(move)):
        if expanded_only and tree["n_child"][i] == 0:
            continue
        path, j = [], i
        while j != 0:
            path.append(int(move[j]))
            j = int(parent[j])
        oe = env_of(start) if isinstance(start, str) else copy_env(start)
        for m in reversed(path):
            oe.make_move(m)
        yield i, oe


def mirror_max_candidates(start, root):
    """the same for a search_mirror tree (Node objects) searched from `start`; a node's child count must be its legal moves"""
    worst, stack = 0, [(root, [])]
    while stack:
        node, path = stack.pop()
        if not node.ch:
            continue
        oe = env_of(start) if isinstance(start, str) else copy_env(start)
        for m in path:
            oe.make_move(m)
        legal, pseudo = raw_counts(oe)
        assert legal == len(node.ch), (path, legal, len(node.ch))
        worst = max(worst, pseudo)
        stack.extend((c, path + [c.mv]) for c in node.ch if c.ch)
    return worst


def max_candidates(start, tree):
    """the most pseudo-legal moves at any expanded node of an oracle tree searched from `start`"""
    return max(raw_counts(oe)[1] for _, oe in node_envs(start, tree))
