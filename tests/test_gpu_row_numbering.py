"""GPU tests (`-m gpu`, through the C ABI) of k_assign_rows - the evaluator row numbering - past one pass of its single
workgroup: more than 16,384 slots, ragged tails behind a full pass, both networks' counts in the packed scan word,
duplicates whose representative was numbered in an earlier pass.  Reference: tests/row_model.number_rows (checked against
brute-force loops by tests/test_row_model_cpu.py).  Every comparison is bit for bit, and row_src - the array the trunk
kernel reads - is read back (xq_engine_read_row_map).

Method: round 0 on caller-provided roots.  The first batch of a search lands on the root, so the pending leaf of a live
game is its root position, which the test chooses.  A DEAD root is a board on which the side to move has no piece:
k_set_roots marks a root without legal moves done, and a game that is done parks no leaf (the CPU oracle confirms zero
legal moves for that board below, before it is used).  Which slots are pending is observed independently of the
numbering: the planes buffer is filled with a sentinel before the launch, and a slot is pending iff the search kernel
overwrote its planes."""
import numpy as np
import pytest

from tests import row_model as rm

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A                       # int16 pattern no plane value has (planes are 0 or bf16 1.0 = 0x3F80)
SIMS = 16


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


@pytest.fixture(scope="module")
def roots():
    """(pool boards [12][90], pool state rows, dead board [90], dead state row): the start position with one piece moved
    (six first moves), each with either side to move - 12 distinct (board, side) pairs with legal moves - and the dead
    root: red's pieces alone, black to move.  All confirmed by the CPU oracle."""
    from chinesechessai_amd import _lib
    from oracle import xq_oracle as xo
    env = xo.OracleEnv()
    env.reset()
    first = env.legal_moves()
    picks = first[::max(1, len(first) // 6)][:6]
    assert len(picks) == 6
    boards, states = [], []

    def state_row(player, rk, bk):
        st = np.zeros(_lib.STATE_WORDS, np.int32)
        st[_lib.S_PLAYER], st[_lib.S_WINNER], st[_lib.S_RED_KING], st[_lib.S_BLACK_KING] = player, _lib.WINNER_NONE, rk, bk
        return st

    for mv in picks:
        e = xo.OracleEnv()
        e.reset()
        e.make_move(mv)
        b = e.board().reshape(90).astype(np.int8)
        rk, bk = int(e.e.red_king), int(e.e.black_king)
        for side in (1, -1):
            chk = xo.OracleEnv()
            chk.set_state(b, side, red_king=rk, black_king=bk)
            assert len(chk.legal_moves()) > 0
            boards.append(b)
            states.append(state_row(side, rk, bk))
    assert len({(b.tobytes(), int(s[_lib.S_PLAYER])) for b, s in zip(boards, states)}) == 12
    env.reset()
    dead = env.board().reshape(90).astype(np.int8)
    dead[dead < 0] = 0                                            # black has no piece left ...
    rk = int(env.e.red_king)
    chk = xo.OracleEnv()
    chk.set_state(dead, -1, red_king=rk, black_king=xo.NO_KING)  # ... and is to move
    assert chk.legal_moves() == [] and (dead > 0).sum() == 16
    return np.stack(boards), np.stack(states), dead, state_row(-1, rk, _lib.NO_KING)


class _Engines:
    """one engine (and its planes buffer) at a time, reused by the cases of one size"""

    def __init__(self):
        self.key, self.eng, self.planes = None, None, None

    def get(self, n_games, vloss=False):
        import torch
        from chinesechessai_amd import _lib
        from chinesechessai_amd.engine import SelfPlayEngine
        if self.key != (n_games, vloss):
            self.close()
            eng = SelfPlayEngine(n_games, sims=SIMS, planes_format=_lib.PLANES_NHWC16_BF16)
            if vloss:
                eng.set_virtual_loss(True)
            self.planes = torch.empty((eng.n_rows, 10 * 9 * 16), dtype=torch.int16, device="cuda")
            self.key, self.eng = (n_games, vloss), eng
        self.eng.set_row_compaction(True)
        self.eng.set_leaf_dedupe(False)
        self.eng.set_pairing(None)
        return self.eng, self.planes

    def close(self):
        if self.eng is not None:
            self.eng.close()
        self.key, self.eng, self.planes = None, None, None


@pytest.fixture(scope="module")
def engines():
    e = _Engines()
    yield e
    e.close()


def _set_roots(eng, roots, live, pos):
    """slot s: pool position pos[s] when live[s], else the dead root"""
    pool_b, pool_s, dead_b, dead_s = roots
    boards = np.where(live[:, None], pool_b[pos], dead_b[None, :]).astype(np.int8)
    states = np.where(live[:, None], pool_s[pos], dead_s[None, :]).astype(np.int32)
    eng.set_roots(boards, states)
    return states[:, 0]                                          # the side to move, per slot


def _round(eng, planes, rnd=0, two=False, ev=None):
    """one search round; returns pending[n_slots] as the planes sentinel shows it"""
    import torch
    from chinesechessai_amd import _lib
    planes.fill_(SENTINEL)
    a, v = (None, None) if ev is None else ev
    if two:
        _lib.check(eng.L.xq_engine_search_round2(eng.h, rnd, _lib.EVAL_PRIORS, a, v, _lib.EVAL_PRIORS, a, v, planes.data_ptr()))
    else:
        _lib.check(eng.L.xq_engine_search_round(eng.h, rnd, _lib.EVAL_PRIORS, a, v, planes.data_ptr()))
    torch.cuda.synchronize()
    written = (planes != SENTINEL)
    pending = written.any(dim=1).cpu().numpy()
    assert bool((written.all(dim=1).cpu().numpy() == pending).all())        # a slot's planes are written whole or not at all
    return pending


def _check(eng, pending, net1=None, dup_of=None, tag=None):
    """leaf_rows, both row maps, both counts and the histories against number_rows(pending, ...)"""
    want_rows, src0, src1, c0, c1 = rm.number_rows(pending, net1=net1, dup_of=dup_of)
    rows = eng.leaf_rows()
    got0, n0 = eng.read_row_map(0)
    got1, n1 = eng.read_row_map(1)
    bad = np.nonzero(rows != want_rows)[0]
    assert len(bad) == 0, "%s: leaf_row differs in %d slots, first slot %d: got %d, want %d" % (
        tag, len(bad), bad[0], rows[bad[0]], want_rows[bad[0]])
    assert (n0, n1) == (c0, c1), "%s: row counts (%d, %d), want (%d, %d)" % (tag, n0, n1, c0, c1)
    assert got0.dtype == np.int32 and np.array_equal(got0, src0), "%s: row_src of network 0 differs" % (tag,)
    assert np.array_equal(got1, src1), "%s: row_src of network 1 differs" % (tag,)
    assert int(eng.row_history()[0][-1]) == c0 + c1, tag
    assert int(eng.row_history_net(0)[0][-1]) == c0 and int(eng.row_history_net(1)[0][-1]) == c1, tag
    return rows


_CASES = [(n, kind) for n in rm.SLOT_COUNTS for kind in rm.MASK_KINDS]


@pytest.mark.parametrize("n,kind", _CASES, ids=["%d-%s" % c for c in _CASES])
def test_rows_are_numbered_in_slot_order_past_one_pass(L, roots, engines, n, kind):
    """One slot per game, n slots, one mask family: leaf_rows(), read_row_map(0) and the count equal number_rows bit for
    bit, row_history()[0][-1] equals the count, network 1 has no rows.  Counts: one vector and its neighbours, one wave
    span and its neighbours, one / two / three passes and their neighbours, ragged tails behind full passes."""
    eng, planes = engines.get(n)
    live = rm.make_mask(kind, n)
    rng = np.random.default_rng(n)
    _set_roots(eng, roots, live, rng.integers(0, 12, n))
    pending = _round(eng, planes)
    assert np.array_equal(pending, live), "a live root parks its root position in round 0, a dead root nothing"
    _check(eng, pending, tag=(n, kind))


@pytest.mark.parametrize("n", (16401, 32785))
def test_duplicates_take_the_row_of_a_representative_in_an_earlier_pass(L, roots, engines, n):
    """Leaf dedupe on, positions drawn from the pool of 12 so that every group's lowest slot lies in pass 0 and further
    members in pass 1 (and 2): same planes <=> same row, rows in the order of each group's lowest slot - 12 rows in all.
    Run twice on the same engine: the second run equals the first (the leaf_dup marks are cleared for the next round)."""
    eng, planes = engines.get(n)
    eng.set_leaf_dedupe(True)
    live, pos = rm.dedupe_assignment(n, 12)
    got = []
    for run in range(2):
        _set_roots(eng, roots, live, pos)
        pending = _round(eng, planes)
        assert np.array_equal(pending, live)
        pl = planes.cpu().numpy()
        keys = [pl[s].tobytes() if pending[s] else None for s in range(n)]      # the group of a slot: its planes, nothing else
        dup = rm.dup_of_groups(pending, keys)
        rows = _check(eng, pending, dup_of=dup, tag=(n, "dedupe", run))
        groups = {}
        for s in np.nonzero(pending)[0]:
            groups.setdefault(keys[s], set()).add(int(rows[s]))
        assert len(groups) == 12 and all(len(r) == 1 for r in groups.values())            # same planes => same row
        assert len({next(iter(r)) for r in groups.values()}) == 12                        # same row => same planes
        assert eng.read_row_map(0)[1] == 12 and eng.read_row_map(0)[0].max() < rm.PASS
        assert (rows[rm.PASS:][pending[rm.PASS:]] >= 0).all()                             # later passes took rows of pass 0
        got.append((rows, eng.read_row_map(0)[0]))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("dedupe", (False, True), ids=("plain", "dedupe"))
@pytest.mark.parametrize("n", (17, 16401, 32785))
def test_two_networks_share_one_scan(L, roots, engines, n, dedupe):
    """xq_engine_search_round2 with a random pairing and random sides: network of a slot = 0 when red is to move or the
    pairing is 0, else 1; both row maps and both counts equal the model, the per-network histories add up to the total,
    and with the dedupe no group - hence no row - spans the two networks."""
    eng, planes = engines.get(n)
    eng.set_leaf_dedupe(dedupe)
    live = rm.make_mask("random50", n)
    rng = np.random.default_rng(n + 1)
    pos = rng.integers(0, 12, n)
    # the network split the CPU test looked at: pairing 1 + black to move exactly where two_network_split says network 1
    want_net1 = rm.two_network_split(n)
    pairing = np.where(want_net1, 1, rng.integers(0, 2, n)).astype(np.uint8)
    pos = np.where(want_net1, pos | 1, np.where(pairing == 1, pos & ~1, pos))      # pool entry 2k: red to move, 2k + 1: black
    eng.set_pairing(pairing)
    side = _set_roots(eng, roots, live, pos)
    net1 = ~((side == 1) | (pairing == 0))
    assert np.array_equal(net1[live], want_net1[live])           # (a dead slot has the dead root's side; it has no row)
    pending = _round(eng, planes, two=True)
    assert np.array_equal(pending, live)
    dup = None
    if dedupe:
        pl = planes.cpu().numpy()
        keys = [(pl[s].tobytes(), bool(net1[s])) if pending[s] else None for s in range(n)]
        dup = rm.dup_of_groups(pending, keys)
    rows = _check(eng, pending, net1=net1, dup_of=dup, tag=(n, "two networks", dedupe))
    (src0, c0), (src1, c1) = eng.read_row_map(0), eng.read_row_map(1)
    assert c0 > 0 and c1 > 0
    assert int(eng.row_history_net(0)[0][-1]) + int(eng.row_history_net(1)[0][-1]) == int(eng.row_history()[0][-1])
    assert not net1[src0].any() and net1[src1].all() and not set(src0.tolist()) & set(src1.tolist())
    # every pending slot's row belongs to its own network and reads planes equal to its own
    for k, src in ((False, src0), (True, src1)):
        sel = np.nonzero(pending & (net1 == k))[0]
        assert (rows[sel] < len(src)).all()
        assert bool((planes[src[rows[sel]].astype(np.int64)] == planes[sel]).all().item())
    eng.set_pairing(None)


@pytest.mark.parametrize("n_games", (2051, 6147))
def test_virtual_loss_slots_rounds_0_and_1(L, roots, engines, n_games):
    """Virtual loss, 8 slots per game: 16,408 slots (one pass + 24) and 49,176 slots (three passes + 24), rounds 0 and 1
    with the hash evaluator in between.  Here the pattern of pending slots is the engine's: round 0 parks one leaf per
    live game (its root, in the game's first slot - asserted), round 1 spreads its 8 simulations over the game's slots.
    Pending comes from the planes sentinel, the expectation from number_rows."""
    from chinesechessai_amd import _lib
    eng, planes = engines.get(n_games, vloss=True)
    K = eng.n_rows // n_games
    assert K == 8 and eng.n_rows in (16408, 49176)
    live = rm.make_mask("random50", n_games)
    _set_roots(eng, roots, live, np.random.default_rng(n_games).integers(0, 12, n_games))
    pending = _round(eng, planes, rnd=0)
    per_game = pending.reshape(n_games, K)
    assert np.array_equal(per_game[:, 0], live) and not per_game[:, 1:].any()
    _check(eng, pending, tag=(n_games, "virtual loss round 0"))
    _lib.check(eng.L.xq_engine_eval_hashnet(eng.h, 7))
    pending = _round(eng, planes, rnd=1, ev=(eng.priors_ptr, eng.values_ptr))
    per_game = pending.reshape(n_games, K)
    assert not per_game[~live].any() and per_game[live].any(axis=1).all()
    spread = per_game[live].sum(axis=1)
    assert spread.max() > 1, "round 1 of a virtual-loss search spreads over several slots"
    assert 0 < pending.sum() < eng.n_rows
    _check(eng, pending, tag=(n_games, "virtual loss round 1"))
