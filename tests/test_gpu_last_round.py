"""GPU tests (`-m gpu`) of xq_engine_set_last_round_visits_only / SelfPlayEngine.set_last_round_visits_only: the last search
round of a ply books its leaf's visits and evaluates nothing.  Everything a game returns - results, outcomes, packed
records - must be what it is with the switch off; the tree after a bare search keeps every visit count and move; terminal
leaves in the last round back up by the rules as always; a one-round ply is left alone; the carry-over counts the roots it
could not carry.  64 games and the exact HashNet evaluator unless a test says otherwise."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = 64
SEEDS = np.arange(4100, 4100 + G, dtype=np.uint32)
PLIES = 24                        # test_games_are_equal: games cut well before the rules' 70th move (its docstring)


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


def _counting_hashnet(salt=0):
    """HashNetEvaluator that keeps row compaction on (priors by slot are served by every layout): the engine then counts
    the rows of every round (row_history)"""
    from chinesechessai_amd.engine import HashNetEvaluator

    class CountingHashNet(HashNetEvaluator):
        def bind(self, engine):
            engine.set_row_compaction(True)
    return CountingHashNet(salt)


def _everything(eng, b):
    """every array a finished batch of games returns: read_results' arrays, the outcomes, the packed records"""
    import torch
    from chinesechessai_amd import distributed as xd
    out = {"r." + k: v for k, v in vars(b).items() if isinstance(v, np.ndarray)}
    out.update({"o." + k: v for k, v in eng.read_game_outcomes().items()})
    t = torch.zeros(eng.n_games * 70 * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    eng.pack_samples(t.data_ptr())
    torch.cuda.synchronize()
    out["records"] = t.cpu().numpy()
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def _play(sims, lrv, carry, ev=None, max_moves=70, setup=None):
    from chinesechessai_amd.engine import SelfPlayEngine
    ev = ev or _counting_hashnet()
    eng = SelfPlayEngine(G, sims=sims, planes_format=ev.planes_format, max_moves=max_moves)
    try:
        if carry is not None:
            eng.set_root_eval_carry(carry)
        if setup:
            setup(eng)
        eng.set_last_round_visits_only(lrv)
        b = eng.play(ev, SEEDS)
        assert eng._lrv_on == lrv
        rows, n = eng.row_history()
        assert len(rows) == n and n % eng.rounds == 0
        return _everything(eng, b), rows.reshape(-1, eng.rounds).astype(np.int64), b
    finally:
        eng.close()


# ---- 1. games ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("sims", [50, 15, 16])
def test_games_are_equal(L, sims, carry):
    """sims 50 (7 rounds, the last of 2 simulations), 15 (2 rounds, last of 7), 16 (2 rounds, last of 8), with and without
    the carry-over: every array, outcome and packed record equal; no ply's last round has a row; fewer rows in all.

    Games of PLIES plies (max_moves), not the rules' 70: "fewer rows" needs a last-round evaluation that nobody uses, and a
    two-round ply under the carry-over has exactly one per game.  Such a ply has ONE visited root child, the last round's
    leaf, so that leaf is the move played and its evaluation is the next root's: one evaluation per position either way -
    with the switch off as the leaf of round 1 (the next round 0 is carried), with it on as the root in round 0 - except
    for the leaf of the game's final ply, which the switch alone leaves out.  At the rules' 70th move that leaf is
    terminal and has no row anyway (measured at full length: 4,480 rows on and off; the test below), so the games are
    cut before it: (PLIES + 1) G rows against PLIES G.  Games that run to the rules' end are compared in the refill,
    playout-cap and full-length tests below."""
    off, rows_off, b = _play(sims, False, carry, max_moves=PLIES)
    on, rows_on, _ = _play(sims, True, carry, max_moves=PLIES)
    assert int(b.error.sum()) == 0 and int(b.n_plies.max()) == PLIES
    _same(on, off, (sims, carry))
    assert rows_on.shape == rows_off.shape == (PLIES, -(-sims // 8))
    assert (rows_on[:, -1] == 0).all() and rows_off[:, -1].sum() > 0
    assert rows_on.sum() < rows_off.sum()
    if sims < 50 and carry and (b.n_plies == PLIES).all():
        assert rows_off.sum() == (PLIES + 1) * G and rows_on.sum() == PLIES * G
    print("sims %d carry %s: rows %d -> %d" % (sims, carry, rows_off.sum(), rows_on.sum()))


@pytest.mark.parametrize("sims,carry", [(15, True), (50, True), (50, False)])
def test_full_length_games_are_equal(L, sims, carry):
    """the same to the rules' end (70 moves, mates, repetitions).  Two-round plies under the carry-over need one row per
    position whichever round evaluates it, and the final ply's leaf is terminal: never more rows, and no fewer either"""
    off, rows_off, b = _play(sims, False, carry)
    on, rows_on, _ = _play(sims, True, carry)
    assert int(b.error.sum()) == 0 and int(b.n_plies.max()) == 70
    _same(on, off, (sims, carry))
    assert (rows_on[:, -1] == 0).all()
    assert rows_on.sum() <= rows_off.sum()
    if sims == 50:
        assert rows_on.sum() < 0.9 * rows_off.sum()
    print("full length, sims %d carry %s: rows %d -> %d" % (sims, carry, rows_off.sum(), rows_on.sum()))


def test_games_are_equal_with_the_network_at_its_defaults(L):
    """A 2-block network on the hand-written kernels with everything automatic (compaction, dedupe, cache, carry-over and
    therefore this elimination) against the plain path: chunked forwards of every slot, no dedupe, no cache, no carry-over,
    every round evaluated."""
    import torch
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    torch.manual_seed(5)
    net = ChessNet(num_blocks=2).eval().cuda()
    ev = TorchNetEvaluator(net)
    eng = SelfPlayEngine(G, sims=50, planes_format=ev.planes_format, max_moves=10)
    seen = []
    orig = eng.search

    def search(*a, **k):
        seen.append(eng._lrv_on)
        return orig(*a, **k)
    eng.search = search
    b = eng.play(ev, SEEDS)
    assert seen and all(seen) and not eng._lrv_on                # automatic: on for these games, off again after them
    assert eng._carry_on and eng.row_compaction and eng.leaf_dedupe
    rows = eng.row_history()[0].reshape(-1, eng.rounds)
    assert (rows[:, -1] == 0).all() and rows[:, 1].sum() > 0
    on = _everything(eng, b)
    eng.close()
    evp = TorchNetEvaluator(ev.inet, chunk=64, leaf_dedupe=False, eval_cache=False)
    engp = SelfPlayEngine(G, sims=50, planes_format=evp.planes_format, max_moves=10)
    engp.set_root_eval_carry(False)
    p = engp.play(evp, SEEDS)
    assert not engp._lrv_on and not engp.row_compaction and int(p.error.sum()) == 0
    off = _everything(engp, p)
    engp.close()
    _same(on, off, "network")


# ---- 2. the tree after a bare search ---------------------------------------------------------------------------------------
def _search_trees(sims, lrv, roots=None, plies_before=0):
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    n = G if roots is None else len(roots[0])
    eng = SelfPlayEngine(n, sims=sims)
    ev = HashNetEvaluator()
    try:
        assert not eng._lrv_on                                   # a bare search never gets it by itself
        if lrv:
            eng.set_last_round_visits_only(True)
        ev.bind(eng)
        if roots is None:
            eng.new_games(SEEDS)
        else:
            eng.set_roots(*roots)
        for _ in range(plies_before):
            eng.search(ev)
            _lib.check(eng.L.xq_engine_play_move(eng.h))
        eng.search(ev)
        mult = np.zeros(n, np.int32)
        _lib.check(eng.L.xq_engine_read_leaves(eng.h, _lib.ptr(np.zeros((n, 90), np.int8)), _lib.ptr(np.zeros(n, np.int32)),
                                               _lib.ptr(np.zeros((n, _lib.MAX_MOVES), np.uint16)), _lib.ptr(np.zeros(n, np.int32)),
                                               _lib.ptr(mult)))
        assert (mult == 0).all()                                 # nothing is pending after a search
        return eng.root_visits(), [eng.read_tree(g) for g in range(n)]
    finally:
        eng.close()


def _compare_trees(off, on, batch_last):
    """the visits-only tree is the other tree without the last round's expansions: same root, same visit_count and move
    on every node both hold.  Returns the number of games whose last round's leaf stayed unexpanded."""
    (m0, v0, n0), t0 = off
    (m1, v1, n1), t1 = on
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and np.array_equal(n0, n1)
    unexpanded = 0
    for g, (a, b) in enumerate(zip(t0, t1)):
        k = len(b["move"])
        assert a["root"] == b["root"] and k <= len(a["move"]), g
        assert np.array_equal(a["visit_count"][:k], b["visit_count"][:k]), g
        assert np.array_equal(a["move"][:k], b["move"][:k]), g
        assert np.array_equal(a["prior"][:k].view(np.uint32), b["prior"][:k].view(np.uint32)), g
        if k < len(a["move"]):
            # the nodes only the plain tree holds are the last leaf's children: created last, never visited
            leaf = np.nonzero((a["n_child"][:k] > 0) & (b["n_child"] == 0))[0]
            assert len(leaf) == 1 and int(a["first_child"][leaf[0]]) == k and int(a["n_child"][leaf[0]]) == len(a["move"]) - k, g
            assert (a["visit_count"][k:] == 0).all() and 0 < int(b["visit_count"][leaf[0]]) <= batch_last, g
            unexpanded += 1
        else:
            assert np.array_equal(a["n_child"], b["n_child"]), g
    return unexpanded


@pytest.mark.parametrize("sims", [15, 50])
def test_tree_after_a_bare_search(L, sims):
    """two plies in, so that the games have separated: root visits equal, every shared node's visit_count and move equal, the
    last round's leaf unexpanded with the switch on, nothing pending"""
    off = _search_trees(sims, False, plies_before=2)
    on = _search_trees(sims, True, plies_before=2)
    assert _compare_trees(off, on, sims - 8 * ((sims - 1) // 8)) == G          # opening positions: no terminal leaf in reach


# ---- 3. terminal leaves in the last round ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sims", [15, 16, 23, 50])
def test_terminal_leaves_in_the_last_round(L, sims):
    """Roots from tests/wide_positions.py through set_roots.  `many_moves` has mating captures among its first choices: at
    15 / 16 simulations every simulation of the last round ends on a terminal leaf (7 / 8 root children with one visit
    each - a non-terminal leaf takes the whole round, so it leaves ONE visited child), at 23 / 50 terminal and parked leaves
    mix.  The other roots keep ordinary slots beside it."""
    from chinesechessai_amd import _lib
    from oracle import xq_oracle as xo
    from tests import wide_positions as wp
    names = ["many_moves", "w64", "heavy_both", "many_moves", "lawful_both_black", "w128", "many_moves", "w65"]
    boards = np.stack([wp.board90(nm) for nm in names])
    st = np.zeros((len(names), _lib.STATE_WORDS), np.int32)
    for i, nm in enumerate(names):
        _, _, _, _, side, rk, bk = wp.entry(nm)
        st[i, _lib.S_PLAYER], st[i, _lib.S_WINNER] = side, _lib.WINNER_NONE
        st[i, _lib.S_RED_KING], st[i, _lib.S_BLACK_KING] = xo.sq(rk), xo.sq(bk)
    off = _search_trees(sims, False, roots=(boards, st))
    on = _search_trees(sims, True, roots=(boards, st))
    batch_last = sims - 8 * ((sims - 1) // 8)
    unexpanded = _compare_trees(off, on, batch_last)
    (_, visits, _), trees = on
    for g, nm in enumerate(names):
        assert int(visits[g].sum()) == sims - 8 and int(trees[g]["visit_count"][trees[g]["root"]]) == sims
    if sims in (15, 16):
        # the terminal path was taken: a round that ends on a parked or a visits-only leaf leaves one visited root child
        mm = [g for g, nm in enumerate(names) if nm == "many_moves"]
        assert all(int((visits[g] > 0).sum()) == batch_last for g in mm), [int((visits[g] > 0).sum()) for g in mm]
        assert all(int(visits[g].max()) == 1 for g in mm)
        assert unexpanded == len(names) - len(mm)
    else:
        assert unexpanded >= len(names) - 3


# ---- 4. one round ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sims", [8, 5])
def test_one_round_plies_are_left_alone(L, sims):
    """sims <= leaf_batch: the only round parks the root and must keep doing so; no child gets a visit and the move choice
    meets NaN probabilities - the reference's error, flag included - with the switch on as with it off"""
    off, rows_off, b = _play(sims, False, False, max_moves=3)
    on, rows_on, _ = _play(sims, True, False, max_moves=3)
    assert (b.error == 1).all()
    _same(on, off, sims)
    assert np.array_equal(rows_on, rows_off) and rows_on[0, 0] == G


# ---- 5. carry-over bookkeeping ---------------------------------------------------------------------------------------------
def test_carry_over_counts_the_roots_it_could_not_carry(L):
    """play() by hand with the carry-over: a game that plays the last round's own leaf has no expansion to carry -
    roots_not_ready() counts exactly those games, and the next ply's round 0 has at most that many rows"""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import SelfPlayEngine
    ev = _counting_hashnet()
    eng = SelfPlayEngine(G, sims=50)
    eng.set_root_eval_carry(True)
    eng.set_last_round_visits_only(True)
    ev.bind(eng)
    eng.new_games(SEEDS)
    assert eng.roots_not_ready() == G
    expected, total = G, 0
    for ply in range(6):
        before = eng.row_history()[1]
        eng.search(ev)
        rows = eng.row_history()[0][-eng.rounds:]
        assert eng.row_history()[1] == before + eng.rounds
        assert rows[0] <= expected and rows[-1] == 0, (ply, rows, expected)
        trees = [eng.read_tree(g) for g in range(G)]
        _lib.check(eng.L.xq_engine_play_move(eng.h))
        chosen = eng.read_results().chosen[:, ply]
        expected = 0
        for g, t in enumerate(trees):
            r = t["root"]
            kids = np.arange(int(t["first_child"][r]), int(t["first_child"][r]) + int(t["n_child"][r]))
            c = kids[t["move"][kids] == chosen[g]]
            assert len(c) == 1 and int(t["visit_count"][c[0]]) > 0, (ply, g)
            expected += int(t["n_child"][c[0]] == 0)
        assert eng.roots_not_ready() == expected, ply
        total += expected
    eng.close()
    assert 0 < total < 6 * G                                     # both kinds of ply end were seen


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_tree_reuse_and_virtual_loss_are_refused_in_both_orders(L):
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import SelfPlayEngine
    for setter in ("set_tree_reuse", "set_virtual_loss"):
        eng = SelfPlayEngine(4, sims=16)
        getattr(eng, setter)(True)
        with pytest.raises(_lib.XqError, match="last-round visits only"):
            eng.set_last_round_visits_only(True)
        assert not eng._lrv_on
        getattr(eng, setter)(False)
        eng.set_last_round_visits_only(True)
        with pytest.raises(_lib.XqError, match="last-round visits only"):
            getattr(eng, setter)(True)
        assert eng._lrv_on
        eng.close()
        # the automatic mode steps aside: a play() after the extension was switched on runs without it
        eng = SelfPlayEngine(4, sims=16, max_moves=2)
        getattr(eng, setter)(True)
        ev = _counting_hashnet()
        ev.row_compaction, ev.deterministic = True, True            # (what the automatic rule looks at)
        seen = []
        orig = eng.search
        eng.search = lambda *a, **k: (seen.append(eng._lrv_on), orig(*a, **k))[1]
        b = eng.play(ev, np.arange(4, dtype=np.uint32))
        assert seen and not any(seen) and int(b.error.sum()) == 0
        eng.close()


# ---- 7. playout cap and refill ---------------------------------------------------------------------------------------------
def test_playout_cap_games_are_equal_and_a_fast_ply_ends_in_round_one(L):
    """fast_sims 16, p 0.25, sims 50, the explicit setter: games and records equal; a fast ply's last round is round 1, so
    round 1 has rows only for the slots at a full ply and rounds 2.. of a ply have the rows they always had"""
    cap = lambda eng: eng.set_playout_cap(0.25, 16, seed=77)
    off, rows_off, b = _play(50, False, False, setup=cap)
    on, rows_on, _ = _play(50, True, False, setup=cap)
    assert int(b.error.sum()) == 0
    _same(on, off, "cap")
    full = b.ply_sims[:, 0] == 50                                # ply 0 of every game: which slots search it fully
    assert 0 < int(full.sum()) < G
    assert rows_off[0].tolist() == [G, G] + [int(full.sum())] * 5
    assert rows_on[0].tolist() == [G, int(full.sum())] + [int(full.sum())] * 4 + [0]
    assert rows_on.sum() < rows_off.sum()


def test_refill_games_are_equal(L):
    """160 games through 64 slots, the explicit setter (refill sessions never get it by themselves)"""
    import torch
    from chinesechessai_amd import distributed as xd
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    seeds = np.arange(9000, 9160, dtype=np.uint32)
    res = []
    for lrv in (False, True):
        eng = SelfPlayEngine(G, sims=15)
        if lrv:
            eng.set_last_round_visits_only(True)
        rec_t = torch.zeros(len(seeds) * 70 * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
        out, plies = eng.play_refill(HashNetEvaluator(), seeds, rec_t.data_ptr())
        torch.cuda.synchronize()
        assert eng._lrv_on == lrv and int(out["error"].sum()) == 0
        out["records"] = rec_t.cpu().numpy()
        out["plies"] = np.array([plies])
        res.append(out)
        eng.close()
    _same(res[1], res[0], "refill")


# ---- 8. a two-network per-slot round ---------------------------------------------------------------------------------------
def test_per_slot_two_network_search(L):
    """one ply in (black to move: pairing-1 slots are searched by network 1), one search(per_slot=True), on against off"""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    got = []
    for lrv in (False, True):
        eng = SelfPlayEngine(G, sims=50)
        if lrv:
            eng.set_last_round_visits_only(True)
        ev0, ev1 = HashNetEvaluator(0), HashNetEvaluator(1)
        eng._bind(ev0, ev1, per_slot=True)
        eng.new_games(SEEDS)
        eng.set_pairing([0, 1] * (G // 2))
        eng.search(ev0, ev1, per_slot=True)
        _lib.check(eng.L.xq_engine_play_move(eng.h))
        eng.search(ev0, ev1, per_slot=True)
        got.append(eng.root_visits())
        eng.close()
    for a, b in zip(*got):
        assert np.array_equal(a, b)
