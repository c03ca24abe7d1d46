"""GPU parity tests (run with `-m gpu` on an MI355X): the HIP path, called through the C ABI
(libxq_hip.so), against the CPU oracle on the same seeded inputs and against the golden vectors
captured from the reference.  Integer/index results and float64 rewards/z are compared
bit-for-bit; only the real-network priors use a tolerance (stated in the test)."""
import json
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(x):
    return struct.pack("<d", float(x))


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


@pytest.fixture(scope="module")
def rules(golden_dir):
    return np.load(os.path.join(golden_dir, "rules_random.npz"))


def _legal_batch(L, boards, player, rk, bk):
    from chinesechessai_amd import _lib
    n = len(player)
    moves = np.zeros((n, 128), np.uint16)
    counts = np.zeros(n, np.int32)
    _lib.check(L.xq_rules_legal_moves(n, _lib.ptr(np.ascontiguousarray(boards, np.int8)),
                                      _lib.ptr(np.ascontiguousarray(player, np.int32)),
                                      _lib.ptr(np.ascontiguousarray(rk, np.int32)),
                                      _lib.ptr(np.ascontiguousarray(bk, np.int32)),
                                      _lib.ptr(moves), _lib.ptr(counts)))
    return moves, counts


def test_legal_moves_golden_rows(L, rules):
    """G1: 5194 positions from the reference -> identical ordered legal-move lists."""
    d = rules
    moves, counts = _legal_batch(L, d["board"], d["player"], d["red_king"], d["black_king"])
    assert np.array_equal(counts, d["nlegal"])
    for i in range(len(counts)):
        assert np.array_equal(moves[i, :counts[i]], d["legal"][i, :counts[i]]), i
    assert counts.max() >= 55


def test_edge_boards(L, golden_dir):
    """Reference unit-test boards (stale king caches) and Appendix-A quirk positions."""
    from chinesechessai_amd import _lib
    cases = json.load(open(os.path.join(golden_dir, "rules_edge.json")))
    n = len(cases)
    boards = np.array([c["board"] for c in cases], np.int8)
    player = np.array([c["player"] for c in cases], np.int32)
    rk = np.array([c["red_king"] for c in cases], np.int32)
    bk = np.array([c["black_king"] for c in cases], np.int32)
    moves, counts = _legal_batch(L, boards, player, rk, bk)
    a, b, f = (np.zeros(n, np.int32) for _ in range(3))
    _lib.check(L.xq_rules_query(n, _lib.ptr(boards), _lib.ptr(player), _lib.ptr(rk), _lib.ptr(bk),
                                _lib.ptr(a), _lib.ptr(b), _lib.ptr(f)))
    for i, c in enumerate(cases):
        assert moves[i, :counts[i]].tolist() == c["legal"], c["name"]
        assert bool(a[i]) == c["in_check_red"] and bool(b[i]) == c["in_check_black"], c["name"]
        assert bool(f[i]) == c["facing"], c["name"]
    # make_move of every legal move of every edge board, one batch
    rows = [(i, m) for i, c in enumerate(cases) for m in c["moves"]]
    nb = len(rows)
    bb = np.stack([boards[i] for i, _ in rows]).copy()
    st = np.zeros((nb, 10), np.int32)
    for j, (i, m) in enumerate(rows):
        st[j, :7] = [player[i], 0, 2, rk[i], bk[i], 0, 0]
    mv = np.array([m["move"] for _, m in rows], np.int32)
    out = _make_move_batch(L, bb, st, mv, None, None)
    for j, (i, m) in enumerate(rows):
        assert bits(out["reward"][j]) == bits(m["reward"]), (cases[i]["name"], m)
        assert bool(out["done"][j]) == m["done"] and bool(out["is_check"][j]) == m["is_check"]
        assert st[j, 2] == m["winner"] and st[j, 3] == m["rk"] and st[j, 4] == m["bk"]
        if m["done"]:
            assert st[j, 7] == m["reason"]


def test_random_boards_vs_oracle(L):
    """20,000 seeded random boards that are NOT restricted to reachable play — random piece
    counts (up to 3 rooks / cannons / knights per side, pieces anywhere, kings possibly outside the
    palace or missing from the cache, stale caches) — legal moves, in-check for both sides, kings
    facing: HIP == oracle.  Then one make_move per board (random legal move, random
    consecutive_checks / no_capture / move_count incl. 69 and 99): reward bits, done, winner,
    reason, caches, next legal moves."""
    from chinesechessai_amd import _lib
    from oracle import xq_oracle as xo
    rng = np.random.RandomState(12345)
    n = 20000
    boards = np.zeros((n, 90), np.int8)
    player = rng.choice([1, -1], size=n).astype(np.int32)
    rk = np.zeros(n, np.int32)
    bk = np.zeros(n, np.int32)
    for i in range(n):
        sqs = rng.permutation(90)
        k = 0
        b = boards[i]
        if rng.rand() < 0.9:
            rsq = (7 + rng.randint(3)) * 9 + 3 + rng.randint(3)
            bsq = rng.randint(3) * 9 + 3 + rng.randint(3)
        else:
            rsq, bsq = int(sqs[88]), int(sqs[89])
        b[rsq] = 1
        b[bsq] = -1 if bsq != rsq else 1
        npieces = rng.randint(0, 26)
        for _ in range(npieces):
            s_ = int(sqs[k]); k += 1
            if b[s_] != 0:
                continue
            t = int(rng.choice([2, 3, 4, 5, 6, 7, 4, 5, 6, 7]))
            b[s_] = t * int(rng.choice([1, -1]))
        mode = rng.rand()
        rk[i] = rsq if mode < 0.85 else (-1 if mode < 0.9 else int(sqs[87]))
        bk[i] = bsq if (mode < 0.85 or mode > 0.95) else (-1 if mode < 0.9 else int(sqs[86]))
    moves, counts = _legal_batch(L, boards, player, rk, bk)
    a, b_, f = (np.zeros(n, np.int32) for _ in range(3))
    _lib.check(L.xq_rules_query(n, _lib.ptr(boards), _lib.ptr(player), _lib.ptr(rk), _lib.ptr(bk),
                                _lib.ptr(a), _lib.ptr(b_), _lib.ptr(f)))
    env = xo.OracleEnv()
    OL = xo.lib()
    pick = np.zeros(n, np.int32)
    st = np.zeros((n, 10), np.int32)
    exp = []
    for i in range(n):
        env.set_state(boards[i], player[i], red_king=rk[i], black_king=bk[i])
        lm = env.legal_moves()
        assert lm == moves[i, :counts[i]].tolist(), i
        assert bool(OL.xqo_is_in_check(env.p, 1)) == bool(a[i]), i
        assert bool(OL.xqo_is_in_check(env.p, -1)) == bool(b_[i]), i
        assert bool(OL.xqo_are_kings_facing(env.p)) == bool(f[i]), i
        mc = int(rng.choice([0, 5, 68, 69, 70]))
        nc = int(rng.choice([0, 3, 98, 99]))
        cc = int(rng.randint(0, 4))
        if lm:
            mv = lm[rng.randint(len(lm))]
        else:
            mv = 0 * 90 + 1          # any move: make_move does not validate (SURVEY.md §8b Errors)
        pick[i] = mv
        st[i, :7] = [player[i], mc, 2, rk[i], bk[i], nc, cc]
        env.set_state(boards[i], player[i], move_count=mc, red_king=rk[i], black_king=bk[i], no_capture=nc,
                      consecutive_checks=cc)
        reward, done, chk = env.make_move(mv)
        e = env.e
        exp.append((reward, done, chk, e.winner, e.end_reason, e.red_king, e.black_king, e.no_capture_count,
                    e.consecutive_checks, env.board().reshape(90).copy(), env.legal_moves() if abs(boards[i][mv % 90]) != 1 else None))
    bb = boards.copy()
    out = _make_move_batch(L, bb, st, pick, None, None)
    for i, (reward, done, chk, winner, reason, erk, ebk, nc2, cc2, eb, nxt) in enumerate(exp):
        assert bits(out["reward"][i]) == bits(reward), (i, out["reward"][i], reward)
        assert bool(out["done"][i]) == done and bool(out["is_check"][i]) == chk, i
        assert st[i, 2] == winner and st[i, 3] == erk and st[i, 4] == ebk and st[i, 5] == nc2 and st[i, 6] == cc2, i
        if done:
            assert st[i, 7] == reason, i
        assert np.array_equal(bb[i], eb), i
        if nxt is not None:
            assert out["next_moves"][i, :out["next_n"][i]].tolist() == nxt, i


def _make_move_batch(L, boards, state, move, pos_hist, chk_hist, n_hist=None, n_chk=None):
    from chinesechessai_amd import _lib
    n = len(move)
    if pos_hist is None:
        stride = 1
        pos_hist = np.zeros((n, 1), np.uint64)
        chk_hist = np.zeros((n, 1), np.uint8)
        n_hist = np.zeros(n, np.int32)
        n_chk = np.zeros(n, np.int32)
    else:
        stride = pos_hist.shape[1]
    out = dict(reward=np.zeros(n, np.float64), done=np.zeros(n, np.int32), is_check=np.zeros(n, np.int32),
               key=np.zeros(n, np.uint64), next_moves=np.zeros((n, 128), np.uint16), next_n=np.zeros(n, np.int32))
    _lib.check(L.xq_rules_make_move(n, _lib.ptr(boards), _lib.ptr(state), _lib.ptr(move), _lib.ptr(pos_hist),
                                    _lib.ptr(n_hist), _lib.ptr(chk_hist), _lib.ptr(n_chk), stride,
                                    _lib.ptr(out["reward"]), _lib.ptr(out["done"]), _lib.ptr(out["is_check"]),
                                    _lib.ptr(out["key"]), _lib.ptr(out["next_moves"]), _lib.ptr(out["next_n"])))
    return out


def test_make_move_golden_trajectories(L, rules):
    """G2: the 48 recorded games replayed ply by ply through xq_rules_make_move (all games of a ply
    in one launch, histories carried by the caller): rewards bit-exact, terminal cascade, caches,
    counters, plus the legal moves of the next position."""
    d = rules
    games = np.unique(d["game"])
    idx = {g: np.where(d["game"] == g)[0] for g in games}
    maxlen = max(len(v) for v in idx.values())
    ng = len(games)
    boards = np.stack([d["board"][idx[g][0]] for g in games]).copy()
    state = np.zeros((ng, 10), np.int32)
    state[:, 0] = 1; state[:, 2] = 2; state[:, 3] = 85; state[:, 4] = 4
    ph = np.zeros((ng, maxlen + 1), np.uint64)
    ch = np.zeros((ng, maxlen + 1), np.uint8)
    nh = np.zeros(ng, np.int32)
    for t in range(maxlen):
        live = [k for k, g in enumerate(games) if t < len(idx[g])]
        rows = [idx[games[k]][t] for k in live]
        b = boards[live].copy()
        s = state[live].copy()
        assert np.array_equal(b, d["board"][rows]), t
        mv = d["move"][rows].astype(np.int32)
        out = _make_move_batch(L, b, s, mv, ph[live].copy(), ch[live].copy(), nh[live].copy(), nh[live].copy())
        for j, (k, r) in enumerate(zip(live, rows)):
            assert bits(out["reward"][j]) == bits(d["reward"][r]), (r, out["reward"][j], d["reward"][r])
            assert bool(out["done"][j]) == bool(d["done"][r]), r
            assert bool(out["is_check"][j]) == bool(d["is_check"][r]), r
            assert s[j, 0] == -d["player"][r] and s[j, 1] == d["move_count"][r] + 1
            assert s[j, 2] == d["winner_after"][r], r
            assert s[j, 3] == d["rk_after"][r] and s[j, 4] == d["bk_after"][r]
            assert s[j, 5] == d["nc_after"][r] and s[j, 6] == d["cc_after"][r]
            if d["done"][r]:
                assert s[j, 7] == d["reason"][r], r
                if d["reason"][r] in (1, 2, 5, 6):
                    assert s[j, 8] == d["reason_side"][r]
                if d["reason"][r] == 8:
                    assert s[j, 9] == d["reason_count"][r]
            # next position's legal moves must equal the next recorded row's list
            if t + 1 < len(idx[games[k]]):
                r2 = idx[games[k]][t + 1]
                assert out["next_moves"][j, :out["next_n"][j]].tolist() == d["legal"][r2, :d["nlegal"][r2]].tolist(), r
            boards[k] = b[j]
            state[k] = s[j]
            ph[k, nh[k]] = out["key"][j]
            ch[k, nh[k]] = out["is_check"][j]
            nh[k] += 1


def test_known_answers_adapter(L, golden_dir):
    """G3 through the host mirror of ChineseChess: 44 ordered initial moves, the 7-ply mate."""
    from chinesechessai_amd import ChineseChess
    from chinesechessai_amd.chess_env import encode_move
    k = json.load(open(os.path.join(golden_dir, "known.json")))
    env = ChineseChess()
    lm = env.get_legal_moves()
    assert [encode_move(m) for m in lm] == k["initial_moves"] and len(lm) == 44
    assert all(isinstance(x, int) for x in lm[0])
    from chinesechessai_amd.chess_env import decode_move
    for mv, r, dn in zip(k["mate_line"], k["mate_rewards"], k["mate_dones"]):
        (board, player), reward, done = env.make_move(decode_move(mv))
        assert reward == r and done == dn
        assert board.dtype == np.int8 and board.shape == (10, 9)
    assert env.winner == 1 and env.end_reason == "将死黑方" and reward == 200 and isinstance(reward, int)
    assert len(env.position_history) == 7 and len(env.check_history) == 7 and len(env.chase_history) == 7


def test_reference_unit_test_boards_adapter(L):
    """The reference's own hand-built test boards, with the results its CURRENT code gives
    (SURVEY.md §4): callers that assign env.board keep the reset king caches."""
    from chinesechessai_amd import ChineseChess
    env = ChineseChess()
    env.board = np.zeros((10, 9), dtype=np.int8)
    env.board[2, 4] = -1
    env.board[8, 4] = 1
    # test_kings_facing.py:13-33 FAILS against the reference's current code for this reason:
    # the stale caches (9,4)/(0,4) see the two kings themselves as blockers
    assert env._are_kings_facing() is False
    env.red_king_pos, env.black_king_pos = (8, 4), (2, 4)
    assert env._are_kings_facing() is True
    env.board[5, 4] = 5
    assert env._are_kings_facing() is False
    # test_reward_system.py:14-41 king capture
    env = ChineseChess()
    env.board = np.zeros((10, 9), dtype=np.int8)
    env.board[0, 4] = -1; env.board[0, 1] = 6; env.board[9, 4] = 1
    env.current_player = 1
    _, reward, done = env.make_move((0, 1, 0, 4))
    assert reward == 100 and done and env.winner == 1 and env.end_reason == "红方吃掉对方将帅"
    assert env.black_king_pos is None
    # test_perpetual_rules.py:20-50
    env = ChineseChess()
    env.check_history = [True, False] * 6
    assert env._check_perpetual_check() is False
    env.check_history = [True] * 11 + [False]
    assert env._check_perpetual_check() is True
    _, reward, done = env.make_move((6, 0, 5, 0))
    assert done and reward == -10 and env.winner == 1 and env.end_reason == "长将判负(黑方)"


def _hash_games(S, seeds, T=1.0, opponent=False, G=None):
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    eng = SelfPlayEngine(len(seeds), sims=S, temperature=T, opponent_mode=opponent)
    b = eng.play(HashNetEvaluator(0), np.array(seeds, np.uint32),
                 opponent_evaluator=HashNetEvaluator(1) if opponent else None)
    eng.close()
    return b


def _cmp_fixture(b, g, r):
    from chinesechessai_amd.chess_env import encode_move
    if r["error"]:
        assert b.error[g] == 1
        return
    assert b.error[g] == 0
    assert b.n_plies[g] == len(r["moves"]), (r["seed"], r["sims"])
    assert b.chosen[g, :b.n_plies[g]].tolist() == r["moves"]
    assert [bits(x) for x in b.step_reward[g, :b.n_plies[g]]] == [bits(x) for x in r["rewards"]]
    assert b.winner[g] == r["winner"] and b.reason[g] == r["reason"]
    assert b.n_samples[g] == r["n_samples"]
    data = b.game_data(g)
    for i, (board, pi, z) in enumerate(data):
        assert bits(z) == bits(r["z"][i]), i
        assert [encode_move(m) for m in pi.keys()] == r["pi_moves"][i]
        assert [bits(p) for p in pi.values()] == [bits(p) for p in r["pi"][i]], i
    if not r["opponent"]:
        for ply in range(b.n_plies[g]):
            n = b.s_n[g, ply]
            assert b.s_moves[g, ply, :n].tolist() == [m for m, _ in r["visits"][ply]]
            assert b.s_counts[g, ply, :n].tolist() == [v for _, v in r["visits"][ply]], (r["seed"], r["sims"], ply)
    import zlib
    crc = 0
    for board, _, _ in data:
        crc = zlib.crc32(board.tobytes(), crc)
    assert crc == r["boards_crc"]


def test_engine_games_vs_reference_golden(L, golden_dir):
    """G4: whole self-play games of the HIP engine with the exact HashNet evaluator against the
    games the unmodified reference played (root visits per ply, sampled moves, rewards, pi, z,
    outcome, CRC of the sample boards) — S in {8,15,16,24,50}, T in {1, .5, .1, argmax},
    arena mode."""
    games = json.load(open(os.path.join(golden_dir, "search_hashnet.json")))
    groups = {}
    for r in games:
        groups.setdefault((r["sims"], r["T"], r["opponent"]), []).append(r)
    for (S, T, opp), rs in groups.items():
        b = _hash_games(S, [r["seed"] for r in rs], T=T, opponent=opp)
        for g, r in enumerate(rs):
            _cmp_fixture(b, g, r)
    slow = os.path.join(golden_dir, "search_hashnet_slow.json")
    if os.path.exists(slow):
        for r in json.load(open(slow)):
            b = _hash_games(r["sims"], [r["seed"]], T=r["T"], opponent=r["opponent"])
            _cmp_fixture(b, 0, r)


def test_engine_games_vs_oracle(L):
    """64 seeded games x S=24 and 32 x S=50: HIP engine == CPU oracle in every recorded field."""
    from oracle import xq_oracle as xo
    for S, n in ((24, 64), (50, 32), (100, 4)):
        seeds = list(range(1000, 1000 + n))
        b = _hash_games(S, seeds)
        for g, seed in enumerate(seeds):
            rc, og = xo.self_play_game(seed, S)
            assert rc == 0 and b.error[g] == 0
            assert og.n_plies == b.n_plies[g] and og.winner == b.winner[g] and og.end_reason == b.reason[g]
            assert list(og.t_move[:og.n_plies]) == b.chosen[g, :og.n_plies].tolist(), (S, seed)
            for i in range(og.n_samples):
                k = og.s_nmoves[i]
                assert list(og.t_visits[i][:k]) == b.s_counts[g, i, :k].tolist(), (S, seed, i)
                assert list(og.s_moves[i][:k]) == b.s_moves[g, i, :k].tolist()
                assert bits(og.s_z[i]) == bits(b.s_z[g, i])
                assert np.array_equal(np.frombuffer(og.s_board[i], dtype=np.int8), b.s_board[g, i])


def test_mcts_search_adapter(L):
    """MCTS(network).search(env) with a reference-style predict_batch object (CallbackEvaluator
    path: leaves read back, priors written) == oracle search on the same position."""
    import zlib
    from chinesechessai_amd import ChineseChess
    from chinesechessai_amd.self_play import MCTS
    from chinesechessai_amd.chess_env import encode_move
    from oracle import xq_oracle as xo

    class HashNet:
        calls = []

        def predict_batch(self, rows):
            self.calls.append(len(rows))
            out = []
            for board, player, legal in rows:
                h0 = zlib.crc32(board.tobytes() + bytes([player & 0xff]))
                probs = {mv: np.float32(((zlib.crc32(bytes(mv), h0) >> 8) % 64 + 1) / 1024) for mv in legal}
                out.append((probs, ((h0 >> 4) % 65 - 32) / 64))
            return out

    env = ChineseChess()
    for mv in [(7, 7, 7, 4), (0, 1, 2, 0), (7, 4, 3, 4)]:
        env.make_move(mv)
    net = HashNet()
    for S in (15, 24, 50):
        vc = MCTS(net, num_simulations=S).search(env)
        oe = xo.OracleEnv()
        for mv in [(7, 7, 7, 4), (0, 1, 2, 0), (7, 4, 3, 4)]:
            oe.make_move(xo.encode_move(mv))
        om, ov = oe.search(S)
        assert [encode_move(m) for m in vc.keys()] == om
        assert list(vc.values()) == ov
        assert sum(vc.values()) == S - 8          # A10: the first batch lands on the root
    assert max(net.calls) == 8                     # rows are passed with the reference's multiplicity


def test_planes_and_network_tolerance(L, golden_dir):
    """G8 + a13: planes written by the search kernel == encode_board of the reference; InferenceNet
    (folded BN, channels-last) vs the reference ChessNet outputs recorded for the same seeded default
    init; and the DEVICE gather + fp32 softmax of consume_eval (neural_network.py:148-169), read back
    with root_priors() after a real search, vs the reference's priors.
    fp32 (library kernels, parity path): |dlogit| <= 2e-4, priors rtol 1e-3.
    bf16 (hand-written kernels): priors rtol 2e-2 = SURVEY.md G8's bound; the measured maximum relative
    error over both nets and all 37 boards is printed by the test (round 2: see DESIGN.md §7), values
    atol 3e-2.  Host softmax of the read-back logits and device softmax must agree to fp32 rounding."""
    import torch
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    d = np.load(os.path.join(golden_dir, "net.npz"))
    n = len(d["players"])
    for tag, seed in (("a", 0), ("b", 1)):
        torch.manual_seed(seed)
        net = ChessNet()
        if tag == "b":
            with torch.no_grad():
                for m in net.modules():
                    if isinstance(m, torch.nn.BatchNorm2d):
                        m.running_mean.uniform_(-0.2, 0.2)
                        m.running_var.uniform_(0.5, 1.5)
                        m.weight.uniform_(0.8, 1.2)
                        m.bias.uniform_(-0.1, 0.1)
        net.eval()
        sd = net.state_dict()
        wsum = np.array([float(sd[k].double().sum()) for k in sorted(sd) if sd[k].dtype.is_floating_point])
        assert np.allclose(wsum, d["wsum_" + tag], rtol=1e-9, atol=1e-9), "seeded init differs from the fixture's"
        assert sum(p.numel() for p in net.parameters()) == int(d["n_params"][0]) == 24634141
        net = net.cuda()
        for dtype, cl, tol_p, tol_v in ((torch.float32, False, 1e-3, 1e-4), (torch.bfloat16, True, 2e-2, 3e-2),
                                        (torch.bfloat16, False, 2e-2, 3e-2)):
            ev = TorchNetEvaluator(net, dtype=dtype, channels_last=cl)
            eng = SelfPlayEngine(n, sims=16, planes_format=ev.planes_format)
            ev.bind(eng)
            st = np.zeros((n, 10), np.int32)
            st[:, 0] = d["players"]; st[:, 2] = 2
            for i in range(n):
                b = d["boards"][i]
                st[i, 3] = int(np.argmax(b.reshape(90) == 1)); st[i, 4] = int(np.argmax(b.reshape(90) == -1))
            eng.set_roots(d["boards"].reshape(n, 90), st)
            _lib.check(eng.L.xq_engine_search_round(eng.h, 0, 0, None, None, ev.planes_ptr()))
            torch.cuda.synchronize()
            planes = ev.x.float().cpu().numpy()[:, :15]
            assert np.array_equal(planes, d["planes"]), "planes != encode_board"
            if cl:
                assert float(ev.x[:, 15].abs().sum()) == 0.0
            kind, a, v = ev.evaluate(eng)
            torch.cuda.synchronize()
            # a leaf's outputs sit in its evaluator row (row compaction; equal positions of the fixture share one)
            rows = eng.leaf_rows()
            assert (rows >= 0).all()
            logits = ev.logits.float().cpu().numpy()[rows]
            values = ev.values.float().cpu().numpy()[rows]
            cmap = ev.inet.column_map                       # compact / padded policy rows: move -> column
            host_p = []
            for i in range(n):
                k = d["nlegal"][i]
                mv = d["legal"][i, :k].astype(np.int64)
                lg = logits[i, cmap[mv].astype(np.int64) if cmap is not None else mv]
                if dtype == torch.float32:
                    assert np.abs(lg - d["logits_" + tag][i, :k]).max() <= 2e-4
                p = np.exp(lg - lg.max()); p /= p.sum()
                host_p.append(p)
                assert np.allclose(p, d["priors_" + tag][i, :k], rtol=tol_p, atol=1e-6), (tag, dtype, i)
                assert abs(values[i] - d["values_" + tag][i]) <= tol_v
            # a13 on the device: a whole search (2 rounds: the root is expanded from the network's output by
            # consume_eval), then the root children's priors as the tree holds them
            eng.set_roots(d["boards"].reshape(n, 90), st)
            eng.search(ev)
            dev_p = eng.root_priors()
            worst = 0.0
            for i in range(n):
                k = d["nlegal"][i]
                ref = d["priors_" + tag][i, :k]
                assert np.allclose(dev_p[i, :k], ref, rtol=tol_p, atol=1e-6), (tag, dtype, i)
                # the hand-written path (bf16 NHWC16) is bit-reproducible, so the two evaluations saw the same
                # logits; PyTorch's library kernels (the fp32 and bf16-NCHW parity paths) are not run-to-run
                # identical: a bf16 logit may flip by one ulp between the two forwards
                assert np.allclose(dev_p[i, :k], host_p[i], rtol=2e-6 if (cl or dtype == torch.float32) else 2e-3,
                                   atol=1e-9), (tag, dtype, i)
                assert (dev_p[i, k:] == 0).all() and abs(float(dev_p[i, :k].sum()) - 1.0) < 1e-5
                worst = max(worst, float(np.max(np.abs(dev_p[i, :k] - ref) / ref)))
            print("a13 device priors vs reference: net %s %s %s: max relative error %.3g (bound %.0e)" % (
                tag, str(dtype).split(".")[-1], "NHWC16" if cl else "NCHW", worst, tol_p))
            eng.close()


def test_fused_conv_kernel_vs_torch(L):
    """csrc/xq_conv.hip: y = relu(conv3x3(x, w) + bias [+ residual]) in NHWC bf16 against an fp32
    torch reference of the same op on the same bf16 inputs.  Tolerance: the kernel rounds conv+bias
    to bf16 once (<= 1 bf16 ulp = 2^-8 relative) and the residual sum once more -> atol 2^-6 on
    values of magnitude <= 4.  Both kernel variants, c_in 16 and 128, odd board counts (tail
    workgroup), with / without residual and ReLU."""
    import torch
    import torch.nn.functional as F
    from chinesechessai_amd import _lib
    torch.manual_seed(1)
    st = torch.cuda.current_stream().cuda_stream
    for variant in (2, 1):
        L.xq_conv3x3_set_variant(variant)
        for cin, G in ((128, 37), (16, 37), (128, 1), (128, 8)):
            x = (torch.randn(G, 10, 9, cin, device="cuda") * 0.5).bfloat16()
            w = (torch.randn(128, cin, 3, 3, device="cuda") / (3 * cin ** 0.5)).bfloat16()
            b = torch.randn(128, device="cuda") * 0.1
            r = (torch.randn(G, 10, 9, 128, device="cuda") * 0.5).bfloat16()
            wk = w.permute(2, 3, 0, 1).reshape(9, 128, cin).contiguous()
            for use_res in (False, True):
                for relu in (1, 0):
                    y = torch.full((G + 1, 10, 9, 128), 7.0, device="cuda", dtype=torch.bfloat16)
                    _lib.check(L.xq_conv3x3_nhwc_bf16(st, x.data_ptr(), wk.data_ptr(), b.data_ptr(),
                                                      r.data_ptr() if use_res else None, y.data_ptr(), G, cin, relu))
                    torch.cuda.synchronize()
                    ref = F.conv2d(x.permute(0, 3, 1, 2).float(), w.float(), b, padding=1)
                    if use_res:
                        ref = ref + r.permute(0, 3, 1, 2).float()
                    if relu:
                        ref = torch.relu(ref)
                    ref = ref.permute(0, 2, 3, 1)
                    assert (y[:G].float() - ref).abs().max().item() <= 2 ** -6 + 2 ** -7 * ref.abs().max().item()
                    assert (y[G] == 7.0).all(), "wrote past the last board"
    L.xq_conv3x3_set_variant(1)
    assert L.xq_conv3x3_nhwc_bf16(st, None, None, None, None, None, 4, 128, 1) == -1
    assert L.xq_conv3x3_nhwc_bf16(st, x.data_ptr(), wk.data_ptr(), b.data_ptr(), None, y.data_ptr(), 4, 64, 1) == -1


def test_fused_heads_kernel_vs_torch(L):
    """k_heads: both 1x1 head convolutions + bias + ReLU, outputs in the (h, w, c) FC layouts, against
    an fp32 torch reference on the same bf16 inputs (atol 2^-7 relative to magnitude <= 4: one bf16
    rounding); odd board counts; nothing written past the end."""
    import torch
    from chinesechessai_amd import _lib
    torch.manual_seed(2)
    st = torch.cuda.current_stream().cuda_stream
    for G in (1, 5, 64):
        x = torch.relu(torch.randn(G, 10, 9, 128, device="cuda") * 0.7).bfloat16()
        w = torch.zeros(64, 128, device="cuda")
        w[:40] = torch.randn(40, 128, device="cuda") / 8
        w = w.bfloat16()
        b = torch.zeros(64, device="cuda")
        b[:40] = torch.randn(40, device="cuda") * 0.2
        P = torch.full((G + 1, 2880), 9.0, device="cuda", dtype=torch.bfloat16)
        V = torch.full((G + 1, 720), 9.0, device="cuda", dtype=torch.bfloat16)
        _lib.check(L.xq_heads_nhwc_bf16(st, x.data_ptr(), w.data_ptr(), b.data_ptr(), P.data_ptr(), V.data_ptr(), G))
        torch.cuda.synchronize()
        ref = torch.relu(x.float().reshape(G, 90, 128) @ w.float().t() + b)            # [G, 90, 64]
        assert (P[:G].float().reshape(G, 90, 32) - ref[..., :32]).abs().max().item() <= 2 ** -7 * max(1.0, ref.abs().max().item())
        assert (V[:G].float().reshape(G, 90, 8) - ref[..., 32:40]).abs().max().item() <= 2 ** -7 * max(1.0, ref.abs().max().item())
        assert (P[G] == 9.0).all() and (V[G] == 9.0).all()


def test_single_launch_trunk_equals_per_layer_kernels(L):
    """csrc/xq_tower.hip (whole trunk in one launch, activations resident in LDS) against (1) the
    per-layer kernels (k_conv3x3_b + k_heads), which the tests above pin to fp32 torch, and (2) an
    fp32 torch evaluation of the same folded bf16 weights with activations rounded to bf16 between
    layers.  Same bf16 storage between layers and the same fp32 accumulation order as the
    per-layer path, except that the skip connection is added in fp32 BEFORE the single bf16
    rounding (the per-layer kernel rounds conv+bias first): bit-identical without residual blocks,
    within a few bf16 ulps (2^-8 relative each) with them.  0, 1, 2 and 6 blocks, odd board counts
    (tail workgroup), and nothing may be written past the last board."""
    import torch
    from chinesechessai_amd.neural_network import ChessNet, InferenceNet
    from chinesechessai_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    # the builds of the trunk kernel: -1 = the library's own choice (round 4: k_tower1wa - one wave per SIMD, the residual
    # tower as one hand-written asm statement - from 2,048 boards up, k_tower16b with 2 boards per workgroup below), 60 =
    # k_tower1wa at any size, 36 / 39 = k_tower16b with 2 / 4 boards per workgroup (v_mfma_f32_16x16x32_bf16, output
    # channels dealt to the MFMA rows 8 per lane, 16-byte epilogue stores, one read / DMA piece per MFMA gap), 0 =
    # k_tower (32x32x16, the comparison build); only the last accumulates in the per-layer kernels' order
    # (bit-identical without residual blocks).  The smallest net on a cold device comes first: that is where a missing
    # DMA wait showed in round 1.
    same_bits = {}
    for variant, blocks, G in ((36, 1, 2), (36, 6, 37), (36, 2, 129), (36, 0, 5), (36, 6, 1), (36, 3, 64), (36, 20, 3), (36, 1, 1024),
                               (39, 1, 2), (39, 6, 37), (39, 2, 129), (39, 0, 5), (39, 6, 1), (39, 3, 64), (39, 20, 3), (39, 1, 1022),
                               (60, 1, 2), (60, 6, 37), (60, 2, 129), (60, 0, 5), (60, 6, 1), (60, 3, 64), (60, 20, 3), (60, 1, 1022),
                               (-1, 1, 2), (-1, 6, 37), (-1, 1, 2049), (-1, 2, 2050),
                               (0, 6, 37), (0, 0, 5), (0, 2, 3)):
        L.xq_tower_set_variant(variant)
        torch.manual_seed(10 + blocks)
        net = ChessNet(num_blocks=blocks).eval()
        for m in net.modules():                                  # non-trivial running statistics
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
        inet = InferenceNet(net.cuda(), fused_tower=False)
        planes = torch.zeros(G, 10, 9, 16, device="cuda", dtype=torch.bfloat16)
        planes[..., :15] = (torch.rand(G, 10, 9, 15, device="cuda") < 0.15).to(torch.bfloat16)
        x = planes.permute(0, 3, 1, 2)
        cur = inet._tower_hip(x).permute(0, 2, 3, 1)
        P0 = torch.empty(G, 2880, device="cuda", dtype=torch.bfloat16)
        V0 = torch.empty(G, 720, device="cuda", dtype=torch.bfloat16)
        _lib.check(L.xq_heads_nhwc_bf16(st, cur.data_ptr(), inet.hip_hw.data_ptr(), inet.hip_hb.data_ptr(),
                                        P0.data_ptr(), V0.data_ptr(), G))
        P1 = torch.full((G + 1, 2880), 9.0, device="cuda", dtype=torch.bfloat16)
        V1 = torch.full((G + 1, 720), 9.0, device="cuda", dtype=torch.bfloat16)
        _lib.check(L.xq_tower_nhwc_bf16(st, planes.data_ptr(), inet.hip_w[0].data_ptr(), inet.hip_wt.data_ptr(),
                                        inet.hip_bt.data_ptr(), inet.hip_hw.data_ptr(), inet.hip_hb.data_ptr(),
                                        P1.data_ptr(), V1.data_ptr(), G, blocks, None, None))
        torch.cuda.synchronize()
        assert P0.abs().max().item() > 0
        assert (P1[G] == 9.0).all() and (V1[G] == 9.0).all()
        if variant in (36, 39, 60, -1):                      # one accumulation order: these builds agree to the bit
            ref = same_bits.setdefault((blocks, G), (P1[:G].clone(), V1[:G].clone(), variant))
            assert torch.equal(ref[0].view(torch.int16), P1[:G].view(torch.int16)), (variant, ref[2], blocks, G)
            assert torch.equal(ref[1].view(torch.int16), V1[:G].view(torch.int16)), (variant, ref[2], blocks, G)
        if blocks == 0 and variant == 0:
            assert torch.equal(P1[:G].view(torch.int16), P0.view(torch.int16)), (blocks, G)
            assert torch.equal(V1[:G].view(torch.int16), V0.view(torch.int16)), (blocks, G)
        # fp32 torch chain on the same bf16 weights, bf16 rounding between layers
        import torch.nn.functional as F
        def cw(i):
            w = inet.hip_w[i].float()                              # [9][128][cin]
            return w.reshape(3, 3, 128, -1).permute(2, 3, 0, 1)
        a = torch.relu(F.conv2d(x.float(), cw(0), inet.hip_b[0], padding=1)).bfloat16().float()
        for i in range(blocks):
            y = torch.relu(F.conv2d(a, cw(1 + 2 * i), inet.hip_b[1 + 2 * i], padding=1)).bfloat16().float()
            a = torch.relu(F.conv2d(y, cw(2 + 2 * i), inet.hip_b[2 + 2 * i], padding=1) + a).bfloat16().float()
        hd = torch.relu(a.permute(0, 2, 3, 1).reshape(G, 90, 128) @ inet.hip_hw.float().t() + inet.hip_hb)
        scale = max(1.0, hd.abs().max().item())
        tol = 2 ** -8 * scale * (2 + blocks)                       # one ulp per rounding point on the path
        for got, name in ((P1[:G], "tower"), (P0, "per-layer")):
            assert (got.float().reshape(G, 90, 32) - hd[..., :32]).abs().max().item() <= tol, (name, blocks, G)
        for got, name in ((V1[:G], "tower"), (V0, "per-layer")):
            assert (got.float().reshape(G, 90, 8) - hd[..., 32:40]).abs().max().item() <= tol, (name, blocks, G)
        assert (P1[:G].float() - P0.float()).abs().max().item() <= tol
        # and through the module: both modes give the same logits / values within the same bound
        inet_f = InferenceNet(net, fused_tower=True)
        la, va = inet(x)
        lb, vb = inet_f(x)
        assert (la.float() - lb.float()).abs().max().item() <= 0.05 * max(1.0, la.float().abs().max().item())
        assert (va.float() - vb.float()).abs().max().item() <= 0.05
    L.xq_tower_set_variant(-1)
    assert L.xq_tower_nhwc_bf16(st, None, None, None, None, None, None, None, None, 4, 6, None, None) == -1


def test_real_network_game_runs_and_invariants(L):
    """Statistical parity with the real net is bounded by H2: here the invariants
    every reference game satisfies — visit totals S-8 per ply (A10), pi sums to 1, z from the
    table, 70-ply cap — on 64 games driven by the bf16 network."""
    import torch
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    torch.manual_seed(0)
    net = ChessNet(num_blocks=2).cuda().eval()
    ev = TorchNetEvaluator(net)
    S = 24
    eng = SelfPlayEngine(64, sims=S, planes_format=ev.planes_format)
    b = eng.play(ev, np.arange(64, dtype=np.uint32))
    assert (b.error == 0).all()
    for g in range(64):
        assert 1 <= b.n_plies[g] <= 70
        for i in range(b.n_samples[g]):
            n = b.s_n[g, i]
            assert b.s_counts[g, i, :n].sum() == S - 8
        if b.reason[g] == 8:
            assert b.n_plies[g] == 70 and b.winner[g] == 0
        data = b.game_data(g)
        assert abs(sum(data[0][1].values()) - 1.0) < 1e-12
    eng.close()


def test_full_size_properties(L):
    """BASELINE config sizes with the exact evaluator: 4096 games x S=15 (C2) — every game must
    equal the oracle's game for its seed (S=15 puts all 7 visits on one child, so all games are
    the same deterministic line: one oracle game checks 4096), plus a checksum-of-checksums over
    sampled moves; 16384 games x S=50 for 3 plies: visit totals and tree sizes."""
    import zlib
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    from oracle import xq_oracle as xo
    G = 4096
    eng = SelfPlayEngine(G, sims=15)
    b = eng.play(HashNetEvaluator(), np.arange(G, dtype=np.uint32))
    eng.close()
    rc, og = xo.self_play_game(0, 15)
    ref = list(og.t_move[:og.n_plies])
    assert (b.n_plies == og.n_plies).all() and (b.winner == og.winner).all()
    # plies 0..68 are seed-independent (one child holds all 7 visits); at ply 69 every child is a
    # terminal leaf (70-ply cap) whose in-round backups spread the visits, so the seed picks
    assert og.n_plies == 70
    assert (b.chosen[:, :69] == np.array(ref[:69], np.uint16)[None, :]).all()
    assert len({zlib.crc32(b.chosen[g, :69].tobytes()) for g in range(G)}) == 1
    assert (b.s_counts[:, :70].astype(np.int64).sum(axis=2) == 7).all()
    for g in (0, 1, 2, 3, 1234, 4095):
        rc, og2 = xo.self_play_game(g, 15)
        assert list(og2.t_move[:70]) == b.chosen[g, :70].tolist()
        k = og2.s_nmoves[69]
        assert list(og2.t_visits[69][:k]) == b.s_counts[g, 69, :k].tolist()
    G = 16384
    eng = SelfPlayEngine(G, sims=50, max_moves=3)
    b = eng.play(HashNetEvaluator(), np.arange(G, dtype=np.uint32))
    eng.close()
    assert (b.n_plies == 3).all() and (b.error == 0).all()
    assert (b.s_counts[:, :3].astype(np.int64).sum(axis=2) == 42).all()
    for g in (0, 1, 777, 16383):
        rc, og = xo.self_play_game(g, 50, max_moves=3)
        assert list(og.t_move[:3]) == b.chosen[g, :3].tolist()
        for i in range(3):
            k = og.s_nmoves[i]
            assert list(og.t_visits[i][:k]) == b.s_counts[g, i, :k].tolist()


def test_refill_every_finished_game_equals_its_oracle_game(L):
    """Refill (the reference's pool does it by construction, self_play.py:404-408): 10 games
    through 4 slots at S = 50 with the exact evaluator.  Seed 2 is the golden game that ends by checkmate at ply
    33 (tests/golden/search_hashnet.json); it is dealt four times so that slots restart at plies 33, 66, 70
    and 103 while their neighbours are mid-game.  Every game — whatever slot and ply it started at — must be
    the oracle's game for its seed, move for move, visit for visit, z bit for bit; and the batch must finish in
    the plies the refill schedule predicts (140), not in 3 lock-step batches (210)."""
    import struct
    import torch
    from chinesechessai_amd import distributed as xd
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    from oracle import xq_oracle as xo
    seeds = np.array([2, 0, 1, 3, 2, 5, 2, 6, 7, 2], dtype=np.uint32)
    G, S, T = 4, 50, len(seeds)
    eng = SelfPlayEngine(G, sims=S)
    rec_t = torch.zeros(T * 70 * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
    out, plies = eng.play_refill(HashNetEvaluator(), seeds, rec_t.data_ptr(), check_every=1)
    rec = xd.records_to_numpy(rec_t).reshape(T, 70)
    eng.close()
    assert (out["error"] == 0).all()
    oracle = {}
    for i, seed in enumerate(seeds):
        if int(seed) not in oracle:
            rc, og = xo.self_play_game(int(seed), S)
            assert rc == 0
            oracle[int(seed)] = og
        og = oracle[int(seed)]
        assert (out["winner"][i], out["reason"][i], out["n_plies"][i], out["n_samples"][i]) == (
            og.winner, og.end_reason, og.n_plies, og.n_samples), (i, seed)
        assert int(rec[i]["valid"].sum()) == og.n_samples and rec[i]["valid"][:og.n_samples].all()
        for j in range(og.n_samples):
            k = og.s_nmoves[j]
            assert int(rec[i, j]["n_moves"]) == k and int(rec[i, j]["chosen"]) == og.t_move[j], (i, j)
            assert rec[i, j]["moves"][:k].tolist() == list(og.s_moves[j][:k])
            assert rec[i, j]["counts"][:k].tolist() == list(og.t_visits[j][:k]), (i, j)
            assert struct.pack("<d", og.s_z[j]) == struct.pack("<d", float(rec[i, j]["z"])), (i, j)
    assert oracle[2].n_plies == 33 and oracle[2].winner == 1                 # the early ending the schedule relies on
    # slot 0: 33 + 33 + 70 = 136; the slots freed at ply 70 take games 6 (33 plies), 7, 8 (70): 140 plies in all
    assert plies == 140, plies


def test_c3_full_size_with_its_own_network(L):
    """BASELINE config C3 end to end under test with its real evaluator: 16,384 concurrent
    games, S = 50, the 6-block bf16 network on the hand-written kernels, 8 plies.  Size-independent properties
    on every game (no errors, 8 samples, every ply's root visits sum to 50 - 8 = 42 [A10], the chosen move is a
    root child with at least one visit, pi sums to 1) and, for a sample of 64 games spread over the batch, an
    oracle replay of the played line: the legal-move list of every sample equals the rules oracle's (order
    included) and the outcome bookkeeping agrees.  The whole run must also be reproducible bit for bit."""
    import torch
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    from oracle import xq_oracle as xo
    torch.manual_seed(0)
    net = ChessNet(num_blocks=6).eval().cuda()
    G, S, P = 16384, 50, 8
    seeds = np.arange(G, dtype=np.uint32)

    def run():
        ev = TorchNetEvaluator(net)
        eng = SelfPlayEngine(G, sims=S, planes_format=ev.planes_format, max_moves=P)
        b = eng.play(ev, seeds)
        eng.close()
        return b

    a = run()
    assert int(a.error.sum()) == 0 and (a.n_plies == P).all() and (a.n_samples == P).all()
    counts = a.s_counts[:, :P].astype(np.int64)
    assert (counts.sum(axis=2) == S - 8).all()
    idx = np.arange(G)
    for i in range(P):
        n = a.s_n[:, i].astype(np.int64)
        pos = (a.s_moves[:, i] == a.chosen[:, i][:, None]) & (np.arange(128)[None, :] < n[:, None])
        assert (pos.sum(axis=1) == 1).all()                                   # the chosen move is one of the root's children
        assert (counts[idx, i, pos.argmax(axis=1)] > 0).all()                 # ... and one that was visited
    for g in np.linspace(0, G - 1, 64).astype(int):
        env = xo.OracleEnv()
        env.reset()
        for i in range(P):
            legal = env.legal_moves()
            k = int(a.s_n[g, i])
            assert a.s_moves[g, i, :k].tolist() == legal and int(a.chosen[g, i]) in legal, (g, i)
            env.make_move(int(a.chosen[g, i]))
        for _, pi, _ in a.game_data(int(g)):
            assert abs(sum(pi.values()) - 1.0) < 1e-9
    b = run()
    assert np.array_equal(a.chosen, b.chosen) and np.array_equal(a.s_counts, b.s_counts)


def test_replay_buffer_vs_reference_semantics(L):
    """the device-resident ReplayBuffer against a restatement of
    trainer.py:22-44 (deque(maxlen), push in game order, np.random.choice indices) and of the batch
    formation trainer.py:313-321 (encode_board(board, 1), float32 rewards) — bit-exact tensors,
    including wrap-around, overflow by more than the capacity in one push, and tuple pushes."""
    import collections
    import torch
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    from chinesechessai_amd.neural_network import ChessNet
    from chinesechessai_amd.replay import ReplayBuffer
    from chinesechessai_amd import distributed as xd

    def play(n, seed0, max_moves):
        eng = SelfPlayEngine(n, sims=16, max_moves=max_moves)
        b = eng.play(HashNetEvaluator(), np.arange(seed0, seed0 + n, dtype=np.uint32))
        rec = torch.zeros(n * _lib.MAX_PLIES * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
        eng.pack_samples(rec.data_ptr())
        torch.cuda.synchronize()
        eng.close()
        return b, rec

    for cap in (500, 90, 5000):
        buf = ReplayBuffer(max_size=cap)
        ref = collections.deque(maxlen=cap)
        for rnd, (n, mm) in enumerate(((7, 70), (5, 13), (3, 70), (9, 30))):
            b, rec = play(n, 100 * rnd, mm)
            pushed = buf.push_records(rec, n)
            k = 0
            for g in range(n):
                for smp in b.game_data(g):
                    ref.append(smp)
                    k += 1
            assert pushed == k and len(buf) == len(ref), (cap, rnd, pushed, k, len(buf), len(ref))
            bs = min(64, len(ref))
            np.random.seed(7 + rnd)
            states, targets = buf.sample_tensors(bs)
            np.random.seed(7 + rnd)
            idx = np.random.choice(len(ref), bs, replace=False)
            exp_states = np.stack([ChessNet.encode_board(ref[i][0], 1) for i in idx]).astype(np.float32)
            exp_targets = torch.FloatTensor([ref[i][2] for i in idx]).unsqueeze(1).numpy()
            assert np.array_equal(states.cpu().numpy(), exp_states), (cap, rnd)
            assert np.array_equal(targets.cpu().numpy(), exp_targets), (cap, rnd)
            np.random.seed(11)
            boards, probs, rewards = buf.sample(min(16, len(ref)))
            np.random.seed(11)
            idx = np.random.choice(len(ref), min(16, len(ref)), replace=False)
            for j, i in enumerate(idx):
                assert np.array_equal(boards[j], ref[i][0]) and rewards[j] == ref[i][2]
                assert list(probs[j].keys()) == list(ref[i][1].keys())
                assert list(probs[j].values()) == list(ref[i][1].values())
        # reference-format tuples pushed from the host
        game = [(ref[i][0], ref[i][1], ref[i][2]) for i in range(min(5, len(ref)))]
        buf.push(game)
        for smp in game:
            ref.append(smp)
        assert len(buf) == len(ref)
        st2, tg2 = buf.sample_tensors(len(ref), indices=np.arange(len(ref)))
        assert np.array_equal(st2.cpu().numpy(), np.stack([ChessNet.encode_board(x[0], 1) for x in ref]).astype(np.float32))
        assert np.array_equal(tg2.cpu().numpy(), torch.FloatTensor([x[2] for x in ref]).unsqueeze(1).numpy())
        with pytest.raises(_lib.XqError):
            buf.sample_tensors(2, indices=np.array([0, len(ref)]))
        buf.close()


def test_real_network_fp32_games_track_the_cpu_reference_algorithm(L):
    """Parity with the real network (statistical, not bitwise).  The engine with the
    fp32 network on the GPU against the CPU oracle driving the SAME weights through the reference's
    predict_batch algorithm (fp32 on CPU torch, NumPy softmax): 6 games x S=24.  fp32 GPU/CPU
    logits differ at the 1e-6 level, which can flip a PUCT near-tie and then the whole game, so the
    assertion is on agreement rates: every game must agree on its first ply's root visits, and
    >= 80 % of all plies must have identical root-visit vectors up to the first divergence."""
    import torch
    from chinesechessai_amd.chess_env import decode_move
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    from oracle import xq_oracle as xo
    torch.manual_seed(5)
    net = ChessNet(num_blocks=2).eval()
    S, G = 24, 6
    cpu_net = net

    def fn(ctx, nrows, boards, players, moves, nmoves, priors, values):
        rows = []
        for i in range(nrows):
            b = np.array([boards[i * 90 + k] for k in range(90)], dtype=np.int8).reshape(10, 9)
            rows.append((b, int(players[i]), [decode_move(moves[i * 128 + j]) for j in range(nmoves[i])]))
        for i, (d, v) in enumerate(cpu_net.predict_batch(rows)):
            for j, p in enumerate(d.values()):
                priors[i * 128 + j] = float(p)
            values[i] = float(v)
        return 0

    cb = xo.EVAL_FN(fn)
    ev_cpu = xo.Evaluator(cb, None)
    gnet = ChessNet(num_blocks=2)
    gnet.load_state_dict(net.state_dict())
    gnet = gnet.cuda().eval()
    ev = TorchNetEvaluator(gnet, dtype=torch.float32)
    eng = SelfPlayEngine(G, sims=S, planes_format=ev.planes_format)
    b = eng.play(ev, np.arange(G, dtype=np.uint32))
    eng.close()
    same = total = 0
    for g in range(G):
        rc, og = xo.self_play_game(g, S, eval_red=ev_cpu)
        assert rc == 0
        k0 = og.s_nmoves[0]
        assert list(og.t_visits[0][:k0]) == b.s_counts[g, 0, :k0].tolist(), g
        for i in range(min(og.n_plies, int(b.n_plies[g]))):
            k = og.s_nmoves[i]
            total += 1
            if list(og.t_visits[i][:k]) == b.s_counts[g, i, :k].tolist() and og.t_move[i] == b.chosen[g, i]:
                same += 1
            else:
                total += min(og.n_plies, int(b.n_plies[g])) - i - 1      # plies after a divergence count as different
                break
    assert same / total >= 0.8, (same, total)


def test_arena_callers_vs_oracle(L):
    """evaluate.py's and compare_models.py's game loops on the engine.  With
    exact evaluators (HashNet salt 0 = red, salt 1 = black) the statistics must equal the ones the
    CPU oracle's games give for the same seeds and temperatures (0.1 / 0.3, NumPy pow tables)."""
    from chinesechessai_amd.arena import evaluate_games, play_match
    from chinesechessai_amd.engine import HashNetEvaluator
    from oracle import xq_oracle as xo
    from tests.test_oracle_search import _salted
    seeds = list(range(300, 312))
    S = 24
    tab01 = np.arange(S + 1, dtype=np.int64) ** (1.0 / 0.1)
    tab03 = np.arange(S + 1, dtype=np.int64) ** (1.0 / 0.3)
    st = evaluate_games(HashNetEvaluator(0), num_games=len(seeds), temperature=0.1, num_simulations=S, seeds=seeds)
    ow, on = [], []
    for sd in seeds:
        rc, g = xo.self_play_game(sd, S, temperature=0.1, pow_table=tab01)
        ow.append(g.winner); on.append(g.n_samples)
    assert st["red_wins"] == ow.count(1) and st["black_wins"] == ow.count(-1) and st["draws"] == ow.count(0)
    assert st["avg_moves"] == float(np.mean(on)) and st["min_moves"] == min(on) and st["max_moves"] == max(on)
    assert len(st["end_reasons"]) == len(seeds) and all(isinstance(x, str) for x in st["end_reasons"])
    res = play_match(HashNetEvaluator(0), HashNetEvaluator(1), num_games=len(seeds), verbose=False,
                     num_simulations=S, seeds=seeds)
    ow, op = [], []
    for sd in seeds:
        rc, g = xo.self_play_game(sd, S, temperature=0.3, eval_black=_salted(1), pow_table=tab03)
        ow.append(g.winner); op.append(g.n_plies)
    assert res["model1_wins"] == ow.count(1) and res["model2_wins"] == ow.count(-1) and res["draws"] == ow.count(0)
    assert res["avg_moves"] == float(np.sum(op) / len(seeds))
    assert set(res) == {"model1_wins", "model2_wins", "draws", "avg_moves", "model1_winrate", "model2_winrate", "draw_rate"}


def test_search_extensions_are_opt_in_and_statistically_sound(L):
    """BASELINE config C5 features that do not exist in the reference (no oracle):
    Dirichlet root noise and a per-ply temperature schedule.  Off by default (all parity tests run
    with them off).  Noise: eta = (P' - (1-eps) P) / eps must be a Dirichlet(alpha) sample —
    non-negative, sums to 1, mean 1/n and variance (1/n)(1-1/n)/(n alpha + 1) over 8,192 games,
    deterministic per seed.  Schedule: plies before the cut-off equal the T = 1 game (oracle), plies
    after it pick the first maximum of the root visits."""
    import zlib
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    from oracle import xq_oracle as xo
    G, alpha, eps = 8192, 0.3, 0.25
    ev = HashNetEvaluator()

    def root_priors(seed, with_noise):
        eng = SelfPlayEngine(G, sims=16)
        if with_noise:
            eng.set_root_noise(alpha, eps, seed)
        eng.new_games(np.arange(G, dtype=np.uint32))
        eng.search(ev)
        p = eng.root_priors()
        eng.close()
        return p

    clean = root_priors(0, False)
    n = 44
    assert (clean[:, n:] == 0).all() and (clean[0] == clean[-1]).all()
    a, b, c = root_priors(1, True), root_priors(1, True), root_priors(2, True)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    eta = (a[:, :n].astype(np.float64) - (1 - eps) * clean[:, :n]) / eps
    assert eta.min() > -1e-5 and np.abs(eta.sum(axis=1) - 1).max() < 1e-4
    assert np.abs(eta.mean(axis=0) - 1.0 / n).max() < 0.004
    var = (1.0 / n) * (1 - 1.0 / n) / (n * alpha + 1)
    assert np.abs(eta.var(axis=0) / var - 1).max() < 0.25
    # games are different across games once the noise is on (per-game streams)
    assert len({zlib.crc32(a[g].tobytes()) for g in range(64)}) == 64

    # temperature schedule: T = 1 for plies < 6, argmax afterwards
    S, cut, NG = 24, 6, 32
    eng = SelfPlayEngine(NG, sims=S)
    bt = eng.play(ev, np.arange(500, 500 + NG, dtype=np.uint32), temperature_schedule=lambda ply: 1.0 if ply < cut else 0.001)
    eng.close()
    for g in range(NG):
        rc, og = xo.self_play_game(500 + g, S, max_moves=cut)
        assert list(og.t_move[:cut]) == bt.chosen[g, :cut].tolist(), g
        for i in range(cut, int(bt.n_plies[g])):
            k = bt.s_n[g, i]
            assert bt.chosen[g, i] == bt.s_moves[g, i, int(np.argmax(bt.s_counts[g, i, :k]))], (g, i)
        pi = list(bt.game_data(g)[cut][1].values())
        assert sorted(pi)[-1] == 1.0 and sum(pi) == 1.0


def test_tree_reuse_is_opt_in_and_consistent(L):
    """Tree reuse (extension; the reference builds a fresh tree every ply): the
    played child's subtree becomes the next ply's tree.  No oracle, so invariants: (1) off by default
    and switching it off again restores the reference games; (2) deterministic; (3) every played
    move is legal and the outcome is the rules oracle's when the moves are replayed on it; (4) the
    root's children carry their visits over: sum of child visits == sims - 8 on a fresh tree (the
    first round lands on the root) and == carried + sims on a kept tree, where carried is the
    played child's own child-visit sum at the previous ply... checked through the stored sample
    counts: the sum never drops below sims - 8 and exceeds it on most plies after the first."""
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    from oracle import xq_oracle as xo
    S, NG = 24, 48
    seeds = np.arange(900, 900 + NG, dtype=np.uint32)
    ev = HashNetEvaluator()

    def run(reuse):
        eng = SelfPlayEngine(NG, sims=S)
        if reuse is not None:
            eng.set_tree_reuse(reuse)
        bt = eng.play(ev, seeds)
        eng.close()
        return bt

    base, off, on1, on2 = run(None), run(False), run(True), run(True)
    for k in ("chosen", "winner", "reason", "n_plies", "s_counts"):
        assert np.array_equal(getattr(base, k), getattr(off, k)), k
        assert np.array_equal(getattr(on1, k), getattr(on2, k)), k
    for g in range(NG):                                     # reference behaviour when off
        rc, og = xo.self_play_game(900 + g, S)
        assert list(og.t_move[:og.n_plies]) == base.chosen[g, :int(base.n_plies[g])].tolist()
    assert not np.array_equal(base.chosen, on1.chosen)
    kept = fresh = 0
    for g in range(NG):
        env = xo.OracleEnv()
        env.reset()
        n = int(on1.n_plies[g])
        for i in range(n):
            legal = env.legal_moves()
            mv = int(on1.chosen[g, i])
            assert mv in legal, (g, i)
            k = int(on1.s_n[g, i])
            assert on1.s_moves[g, i, :k].tolist() == legal, (g, i)
            tot = int(on1.s_counts[g, i, :k].sum())
            assert tot >= S - 8, (g, i, tot)
            if i > 0:
                kept += tot > S - 8
                fresh += tot == S - 8
            env.make_move(mv)
        w = int(env.e.winner)
        assert int(on1.winner[g]) == (0 if w == xo.WINNER_NONE else w), g
    assert kept > 4 * fresh, (kept, fresh)                 # the sampled move almost always had been expanded


def _vl_search_mirror(S, leaf_batch=8):
    """One MCTS.search from the start position WITH virtual loss as the engine defines it (a pending visit counts as N + 1,
    W - 1 on every node of its path; a round's pending leaves are expanded and backed up in the order they were reached),
    restated in Python: tests/search_mirror.py.  Rules and the evaluator: the oracle env / HashNet."""
    from oracle import xq_oracle as xo
    from tests.search_mirror import Node, hashnet_evaluate, search_mirror
    env = xo.OracleEnv()
    env.reset()
    return search_mirror(env, Node(), S, leaf_batch, virtual_loss=True, evaluate=hashnet_evaluate)


def test_virtual_loss_is_opt_in_and_matches_its_restatement(L):
    """Virtual loss (extension; the reference freezes the tree inside a round,
    Appendix A10).  Off by default (every parity test above runs without it).  On: (1) one search
    from the start position equals a Python restatement of the same rule, visit for visit, for
    S = 16, 24, 50; (2) no pending visits are left after a search and the rounds now expand several
    leaves (arena grows by far more than one expansion per round); (3) whole games are
    deterministic, play legal moves only and end as the rules oracle says; (4) the host-callback
    evaluator path refuses to run with it."""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import CallbackEvaluator, HashNetEvaluator, SelfPlayEngine
    from oracle import xq_oracle as xo
    ev = HashNetEvaluator()
    for S in (16, 24, 50):
        eng = SelfPlayEngine(4, sims=S)
        eng.set_virtual_loss(True)
        assert eng.n_rows == 4 * 8
        eng.new_games(np.arange(4, dtype=np.uint32))
        eng.search(ev)
        moves, visits, n = eng.root_visits()
        nodes, vl = eng.tree_stats()
        eng.close()
        mm, mv, root = _vl_search_mirror(S)
        assert n[0] == len(mm) and moves[0, :n[0]].tolist() == mm
        assert visits[0, :n[0]].tolist() == mv, (S, visits[0, :n[0]].tolist(), mv)
        assert (visits == visits[0]).all() and (vl == 0).all()
        rounds = (S + 7) // 8
        assert nodes[0] > 1 + 44 * 2 * (rounds - 1)             # > 2 expansions per round after the first
    S, NG = 24, 32
    seeds = np.arange(1300, 1300 + NG, dtype=np.uint32)

    def run():
        eng = SelfPlayEngine(NG, sims=S)
        eng.set_virtual_loss(True)
        bt = eng.play(ev, seeds)
        eng.close()
        return bt

    a, b = run(), run()
    for k in ("chosen", "winner", "reason", "n_plies", "s_counts"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for g in range(NG):
        env = xo.OracleEnv()
        env.reset()
        for i in range(int(a.n_plies[g])):
            legal = env.legal_moves()
            k = int(a.s_n[g, i])
            assert a.s_moves[g, i, :k].tolist() == legal and int(a.chosen[g, i]) in legal, (g, i)
            assert int(a.s_counts[g, i, :k].sum()) == S - 8, (g, i)      # the first round still lands on the root
            env.make_move(int(a.chosen[g, i]))
        w = int(env.e.winner)
        assert int(a.winner[g]) == (0 if w == xo.WINNER_NONE else w), g

    class Net:
        def predict_batch(self, rows):
            return [({m: 1.0 / len(legal) for m in legal}, 0.0) for _, _, legal in rows]
    eng = SelfPlayEngine(2, sims=16)
    eng.set_virtual_loss(True)
    eng.new_games(np.arange(2, dtype=np.uint32))
    cb = CallbackEvaluator(Net())
    cb.bind(eng)
    with pytest.raises(_lib.XqError):
        eng.search(cb)
    eng.close()


def test_extensions_with_the_real_network(L):
    """Tree reuse + virtual loss + root noise together on the bf16 network path (8 evaluator rows per
    game): games complete without errors, only legal moves are played (rules oracle replay), pi of
    every sample sums to 1 and the run is repeatable bit for bit: since round 2 every kernel of the network
    forward is hand-written with a fixed accumulation order (the library stream-K GEMM of round 1, whose split
    varies from launch to launch, is gone: csrc/xq_policy.hip)."""
    import torch
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    from oracle import xq_oracle as xo
    torch.manual_seed(3)
    net = ChessNet(num_blocks=2).cuda().eval()
    NG, S = 48, 24
    seeds = np.arange(77, 77 + NG, dtype=np.uint32)

    def run():
        ev = TorchNetEvaluator(net)
        eng = SelfPlayEngine(NG, sims=S, planes_format=ev.planes_format, max_moves=30)
        eng.set_tree_reuse(True)
        eng.set_virtual_loss(True)
        eng.set_root_noise(0.3, 0.25, seed=5)
        assert eng.n_rows == NG * 8
        bt = eng.play(ev, seeds)
        nodes, vl = eng.tree_stats()
        eng.close()
        assert (vl == 0).all() and nodes.max() < 65472
        return bt

    a, b = run(), run()
    assert np.array_equal(a.chosen, b.chosen) and np.array_equal(a.s_counts, b.s_counts)
    assert np.array_equal(a.s_z.view(np.int64), b.s_z.view(np.int64))
    assert int(a.error.sum()) == 0 and (a.n_plies == 30).all()
    for g in range(NG):
        env = xo.OracleEnv()
        env.reset()
        for i in range(int(a.n_plies[g])):
            legal = env.legal_moves()
            k = int(a.s_n[g, i])
            assert a.s_moves[g, i, :k].tolist() == legal and int(a.chosen[g, i]) in legal, (g, i)
            env.make_move(int(a.chosen[g, i]))
        for _, pi, _ in a.game_data(g):
            assert abs(sum(pi.values()) - 1.0) < 1e-9


def test_reachable_policy_columns_give_the_same_priors(L, golden_dir):
    """Compact policy head (2,294 of 8,100 columns; the default since round 2) vs the full head on the network fixture
    positions: BIT-identical legal-move priors - k_policy_fc accumulates every output element in one fixed fp32 chain
    over k, whatever the tile position, the column count or the row count (csrc/xq_policy.hip), so dropping the dead
    columns cannot move a single logit; plus 20,000 random boards whose legal moves (HIP) all map to a column."""
    import torch
    from chinesechessai_amd import _lib
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet, reachable_policy_columns
    d = np.load(os.path.join(golden_dir, "net.npz"))
    n = len(d["players"])
    torch.manual_seed(0)
    net = ChessNet().cuda().eval()
    pri = {}
    for mode in ("all", "reachable"):
        ev = TorchNetEvaluator(net, policy_columns=mode)
        eng = SelfPlayEngine(n, sims=16, planes_format=ev.planes_format)
        ev.bind(eng)
        st = np.zeros((n, 10), np.int32)
        st[:, 0] = d["players"]; st[:, 2] = 2
        for i in range(n):
            b = d["boards"][i].reshape(90)
            st[i, 3] = int(np.argmax(b == 1)); st[i, 4] = int(np.argmax(b == -1))
        eng.set_roots(d["boards"].reshape(n, 90), st)
        eng.search(ev)                       # 2 rounds; the root is expanded with the network's priors
        pri[mode] = eng.root_priors()
        assert ev.logits.shape[1] == (8256 if mode == "all" else 2304)          # rows padded to the FC kernel's 192
        eng.close()
    for i in range(n):
        k = d["nlegal"][i]
        assert np.array_equal(pri["all"][i, :k].view(np.int32), pri["reachable"][i, :k].view(np.int32)), i
        assert abs(pri["reachable"][i, :k].sum() - 1) < 1e-3
    cols, cmap = reachable_policy_columns()
    rng = np.random.RandomState(99)
    boards = np.zeros((20000, 90), np.int8)
    for i in range(20000):
        sq = rng.permutation(90)[:rng.randint(2, 30)]
        boards[i, sq] = rng.choice([1, 2, 3, 4, 5, 6, 7, -1, -2, -3, -4, -5, -6, -7], size=len(sq))
    player = rng.choice([1, -1], size=20000).astype(np.int32)
    nk = np.full(20000, -1, np.int32)
    moves, counts = _legal_batch(L, boards, player, nk, nk)
    for i in range(20000):
        assert (cmap[moves[i, :counts[i]].astype(np.int64)] >= 0).all(), i


def test_self_play_api_mirror_vs_reference_golden(L, golden_dir):
    """The reference's call surface end to end: self_play_game under a seeded
    GLOBAL NumPy stream must return the reference's game (tuples of int8 board, {move: float64},
    float z; winner; end_reason string) and leave the stream where the reference leaves it;
    parallel_self_play returns the golden games in game order; S <= 8 raises ValueError."""
    from chinesechessai_amd.engine import HashNetEvaluator
    from chinesechessai_amd.self_play import InterruptedWithResults, parallel_self_play, self_play_game
    from chinesechessai_amd.chess_env import encode_move, format_end_reason
    games = {(r["seed"], r["sims"], r["T"], r["opponent"]): r for r in json.load(open(os.path.join(golden_dir, "search_hashnet.json")))}
    for key in ((2, 50, 1.0, False), (0, 15, 1.0, False), (5, 24, 0.5, False), (8, 24, 1.0, True)):
        r = games[key]
        np.random.seed(r["seed"])
        data, winner, reason = self_play_game(HashNetEvaluator(0), temperature=r["T"], num_simulations=r["sims"],
                                              opponent_network=HashNetEvaluator(1) if r["opponent"] else None)
        after = np.random.random_sample()
        np.random.seed(r["seed"])
        np.random.random_sample(len(r["moves"]))
        assert after == np.random.random_sample(), "global stream position differs from the reference's"
        assert winner == r["winner"] and len(data) == r["n_samples"]
        assert reason == (format_end_reason(r["reason"], r["reason_side"], r["reason_count"]) or "未知原因")
        for i, (board, pi, z) in enumerate(data):
            assert board.dtype == np.int8 and board.shape == (10, 9) and isinstance(z, float)
            assert bits(z) == bits(r["z"][i])
            assert [encode_move(m) for m in pi] == r["pi_moves"][i]
            assert [bits(p) for p in pi.values()] == [bits(p) for p in r["pi"][i]]
            assert all(isinstance(p, np.float64) for p in pi.values())
    res = parallel_self_play(HashNetEvaluator(0), 4, temperature=1.0, num_simulations=50, num_workers=4, seeds=[0, 1, 2, 3])
    assert len(res) == 4
    for g, (data, winner, reason) in enumerate(res):
        r = games[(g, 50, 1.0, False)]
        assert winner == r["winner"] and [bits(z) for _, _, z in data] == [bits(z) for z in r["z"]]
    assert res[2][2] == "将死黑方" and res[0][2] == "超过70步判和"
    with pytest.raises(ValueError):
        self_play_game(HashNetEvaluator(0), num_simulations=8)
    assert parallel_self_play(HashNetEvaluator(0), 2, num_simulations=8, seeds=[0, 1]) == []     # failed games are dropped
    assert issubclass(InterruptedWithResults, Exception) and InterruptedWithResults([1]).results == [1]


def test_bench_contract_line(L, monkeypatch, capsys):
    """bench.py's one JSON line on a tiny workload, in process: every key of the driver's contract,
    the two objects this tier adds (`roofline`, and with `--full` `cpu_baseline`), and the same again through the
    RCCL code path with a single rank (init, all-gather of the sample records, barrier, MAX
    all-reduce of the time)."""
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(root)
    bench = importlib.import_module("bench")
    base = ["bench.py", "--games", "256", "--sims", "16", "--blocks", "2", "--steps", "1", "--warmup", "0"]

    def run(argv, env=None):
        monkeypatch.setattr(sys, "argv", argv)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        bench.main()
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        return json.loads(lines[0])

    d = run(base + ["--full"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "games/s" and d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 0
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "bf16" and d["data"].startswith("synthetic") and "workload" in d["config"]
    assert abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["achieved"] > 0 and "traffic" in r
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "games/s" and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    assert d["games"]["errors"] == 0
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    d2 = run(base + ["--no-cpu-baseline"], env={"XQ_BENCH_FORCE_DIST": "1", "RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1",
                                                "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    assert d2["n_gpus"] == 1 and "cpu_baseline" not in d2 and d2["value"] > 0
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()


def test_bench_plain_run_is_lean_and_dumps_repeatable_outputs(L, monkeypatch, capsys, tmp_path):
    """A plain bench.py run carries none of the figures that take runs of their own (`value_*`, `cpu_baseline`: --full);
    --steps sets the timed steps; --dump-outputs writes the last timed step's sample records as float32 / float64
    arrays that are the same from run to run and agree with the games the engine reports."""
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(root)
    bench = importlib.import_module("bench")
    G = 300                                                    # more than bench.DUMP_SAMPLE_GAMES: the seeded sample is taken
    assert G > bench.DUMP_SAMPLE_GAMES
    dumps = []
    for rep in range(2):
        out = tmp_path / ("dump%d" % rep)
        monkeypatch.setattr(sys, "argv", ["bench.py", "--games", str(G), "--sims", "16", "--blocks", "2", "--steps", "2",
                                          "--warmup", "0", "--dump-outputs", str(out)])
        bench.main()
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["steps"] == 2 and abs(d["value"] - G / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
        assert "cpu_baseline" not in d and not [k for k in d if k.startswith("value_")] and "roofline" in d
        dumps.append({f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))})
    a, b = dumps
    assert sorted(a) == sorted(b) and {"z", "valid", "player", "n_moves", "chosen", "scalar_games", "sample_games", "sample_board",
                                       "sample_moves", "sample_counts", "outcome_n_samples"} <= set(a)
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert a["z"].shape == (G, 70) and a["sample_counts"].shape == (bench.DUMP_SAMPLE_GAMES, 70, 128)
    assert np.array_equal(a["scalar_games"], np.arange(G)) and np.array_equal(a["valid"].sum(axis=1), a["outcome_n_samples"])
    si = a["sample_games"].astype(np.int64)
    assert len(set(si.tolist())) == bench.DUMP_SAMPLE_GAMES and (np.diff(si) > 0).all() and si.max() < G
    v = a["valid"][si] != 0
    assert (a["sample_counts"].sum(axis=2)[v] == 16 - 8).all() and (a["sample_counts"][~v] == 0).all()   # S - 8 visits per ply (A10)
    assert ((a["sample_moves"] != 0).sum(axis=2) <= a["n_moves"][si]).all() and (np.abs(a["sample_board"]) <= 7).all()
    assert np.isfinite(a["z"]).all() and (a["z"][a["valid"] == 0] == 0).all()


# ------------------------------------------------------------------------------------------------------
# round 2: a8, repetition, private predicates, reference-written trainer-side fixtures
# ------------------------------------------------------------------------------------------------------
def _mirror_env(p):
    from chinesechessai_amd import ChineseChess
    from chinesechessai_amd.chess_env import _pos
    env = ChineseChess()
    env.board = np.array(p["board"], np.int8).reshape(10, 9)
    env.current_player = p["player"]
    env.red_king_pos, env.black_king_pos = _pos(p["red_king"]), _pos(p["black_king"])
    env.move_count = p.get("move_count", 0)
    env.no_capture_count = p.get("no_capture", 0)
    return env


def test_threatened_pieces_chase_history_and_private_predicates(L, golden_dir):
    """a8 and the private predicates (VERDICT r01 missing #3, weak #9) against tests/golden/rules_extra.json, which
    the unmodified reference generated: xq_rules_threatened_pieces in one batch through the C ABI for every ply of
    the chase games and both sides of the probe positions; the mirror's lazily filled chase_history along whole
    games; _check_checkmate / _check_stalemate / _is_move_suicide / _get_position_hash on the mirror."""
    from chinesechessai_amd import _lib
    from chinesechessai_amd.chess_env import decode_move
    d = json.load(open(os.path.join(golden_dir, "rules_extra.json")))
    # (1) batch through the C ABI: positions AFTER each move (the oracle env applies the move), side = mover
    boards, side, rk, bk, want = [], [], [], [], []
    for game in d["chase"]:
        env = None
        from chinesechessai_amd import ChineseChess
        env = ChineseChess()
        for p in game:
            assert env.board.reshape(90).tolist() == p["board"] and env.current_player == p["player"]
            env.make_move(decode_move(p["move"]))
            boards.append(env.board.reshape(90).copy()); side.append(p["player"])
            rk.append(-1 if env.red_king_pos is None else env.red_king_pos[0] * 9 + env.red_king_pos[1])
            bk.append(-1 if env.black_king_pos is None else env.black_king_pos[0] * 9 + env.black_king_pos[1])
            want.append(p["chase"])
        # the mirror's own chase_history, filled lazily on first read, == the reference's per-ply lists
        got = [[(a[0] * 9 + a[1]) * 90 + b[0] * 9 + b[1] for a, b in e] for e in env.chase_history]
        assert got == [p["chase"] for p in game]
    for t in d["threats"]:
        for s, key in ((1, "red"), (-1, "black")):
            boards.append(np.array(t["board"], np.int8)); side.append(s); rk.append(t["red_king"]); bk.append(t["black_king"])
            want.append(t[key])
    n = len(side)
    pairs = np.zeros((n, 128), np.uint16)
    counts = np.zeros(n, np.int32)
    _lib.check(L.xq_rules_threatened_pieces(n, _lib.ptr(np.ascontiguousarray(np.stack(boards), np.int8)),
                                            _lib.ptr(np.array(side, np.int32)), _lib.ptr(np.array(rk, np.int32)),
                                            _lib.ptr(np.array(bk, np.int32)), _lib.ptr(pairs), _lib.ptr(counts)))
    for i in range(n):
        assert pairs[i, :counts[i]].tolist() == want[i], i
    assert sum(len(w) for w in want) > 150
    # (2) predicates on the mirror
    mates = 0
    for p in d["predicates"]:
        env = _mirror_env(p)
        assert env._check_checkmate() == p["checkmate"] and env._check_stalemate() == p["stalemate"], p["name"]
        for mv, expect in p["suicide"][:12]:
            assert env._is_move_suicide(*decode_move(mv)) == expect, (p["name"], mv)
        assert env._is_protected(0, 0, 1) is False
        mates += p["checkmate"]
    assert mates >= 1
    a, b = _mirror_env(d["predicates"][0]), _mirror_env(d["predicates"][0])
    assert a._get_position_hash() == b._get_position_hash()
    b.current_player = -b.current_player
    assert a._get_position_hash() != b._get_position_hash()


def test_repetition_draw_with_injected_history(L, golden_dir):
    """chess_env.py:598-605 has no positive case in legal play (Appendix A7: the entry a move appends carries the
    MOVER's byte, the test hashes with the NEXT player's); the reference's cases inject k copies of the hash the
    test will compute.  Through the mirror (position_history = k keys from _get_position_hash of the probe
    position) and in one batch through xq_rules_make_move: draw (reason 3, reward 0 as a Python int, winner 0) for
    k >= 3, the reference's ordinary outcome for k = 2."""
    from chinesechessai_amd.chess_env import decode_move
    d = json.load(open(os.path.join(golden_dir, "rules_extra.json")))
    draws = 0
    for r in d["repetition"]:
        probe = _mirror_env(dict(board=r["key_board"], player=r["key_player"], red_king=r["red_king"], black_king=r["black_king"]))
        h = probe._get_position_hash()
        env = _mirror_env(r)
        env.position_history = [h] * r["copies"]
        _, reward, done = env.make_move(decode_move(r["move"]))
        assert (float(reward), done, 2 if env.winner is None else env.winner) == (r["reward"], r["done"], r["winner"]), r
        assert len(env.position_history) == r["n_hist_after"] and env._check_draw_by_repetition() == r["repetition_now"]
        if r["reason"] == 3:
            assert env.end_reason == "三次重复局面判和" and isinstance(reward, int) and reward == 0
            draws += 1
    assert draws == 12


def test_replay_buffer_vs_reference_trace(L, golden_dir):
    """(f-1) pinned to the reference class itself: tests/golden/trainer_io.npz holds the
    games pushed into trainer.ReplayBuffer(max_size=40) and, after every second push, what its sample(bs) returned
    under np.random.seed(s) plus the batch trainer.py:313-321 forms from it (encode_board(board, 1), FloatTensor
    rewards) — generated by the unmodified reference.  The device ring must return the same boards, rewards,
    move-probability keys and bit-identical state / target tensors."""
    import torch
    from chinesechessai_amd.chess_env import decode_move
    from chinesechessai_amd.replay import ReplayBuffer
    d = np.load(os.path.join(golden_dir, "trainer_io.npz"))
    buf = ReplayBuffer(max_size=int(d["capacity"][0]))
    traces = {int(d["t%d_meta" % t][0]): t for t in range(int(d["n_traces"][0]))}
    for g in range(int(d["n_games"][0])):
        boards, zs, nm = d["g%d_boards" % g], d["g%d_z" % g], d["g%d_nmoves" % g]
        moves, probs = d["g%d_moves" % g], d["g%d_probs" % g]
        off, game = 0, []
        for i in range(len(zs)):
            k = int(nm[i])
            game.append((boards[i].reshape(10, 9), {decode_move(m): np.float64(p) for m, p in zip(moves[off:off + k], probs[off:off + k])},
                         float(zs[i])))
            off += k
        buf.push(game)
        if g in traces:
            t = traces[g]
            after, size, bs, seed = (int(v) for v in d["t%d_meta" % t])
            assert len(buf) == size
            np.random.seed(seed)
            b, p, r = buf.sample(bs)
            assert np.array_equal(np.stack([x.reshape(90) for x in b]), d["t%d_boards" % t])
            assert np.array_equal(np.array(r, np.float64).view(np.int64), d["t%d_rewards" % t].view(np.int64))
            fp = d["t%d_first_probs" % t]
            assert [(m[0] * 9 + m[1]) * 90 + m[2] * 9 + m[3] for m in p[0].keys()] == fp[:, 0].astype(int).tolist()
            # host-pushed tuples come back as they were pushed (trainer.py:27-42 keeps the tuples themselves)
            assert np.array_equal(np.array(list(p[0].values()), np.float64).view(np.int64),
                                  np.ascontiguousarray(fp[:, 1], dtype=np.float64).view(np.int64))
            np.random.seed(seed)
            states, targets = buf.sample_tensors(bs)
            assert np.array_equal(np.packbits(states.cpu().numpy().astype(np.uint8)), d["t%d_states_bits" % t])
            assert set(np.unique(states.cpu().numpy())) <= {0.0, 1.0}
            assert np.array_equal(targets.cpu().numpy().view(np.int32), d["t%d_targets" % t].view(np.int32))
    buf.close()


def test_on_disk_formats_vs_reference_written_files(L, golden_dir, tmp_path):
    """(f-3): engine output -> formats.append_best_games -> a file the reference's viewer parses exactly like the one
    the reference's own Trainer._save_best_games wrote (tests/golden/best_games_ref.pkl: the golden seed-2 S=50 game
    and the seed-0 S=15 game through the unmodified self_play_game + _save_best_games).  Same keys, same game_data
    (boards, move -> float64 probability in legal-move order, z bit for bit), winner, moves, type; replayed the way
    view_best_games.py:193-213 replays it (arg-max move of every sample through ChineseChess.make_move) the two
    files give the same board sequence.  Checkpoint: formats.save_checkpoint has the structure Trainer.save_model
    wrote (tests/golden/checkpoint_struct.json)."""
    import pickle
    import torch
    from chinesechessai_amd import ChineseChess, formats
    from chinesechessai_amd.engine import HashNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    from chinesechessai_amd.self_play import parallel_self_play
    ref_games = pickle.load(open(os.path.join(golden_dir, "best_games_ref.pkl"), "rb"))
    assert [g["moves"] for g in ref_games] == [33, 70] and [g["total_games"] for g in ref_games] == [200, 300]
    path = tmp_path / "data" / "best_games.pkl"
    for (seed, sims), total in (((2, 50), 200), ((0, 15), 300)):
        res = parallel_self_play(HashNetEvaluator(), 1, temperature=1.0, num_simulations=sims, seeds=np.array([seed], np.uint32))
        formats.append_best_games(str(path), formats.best_games_from_results(res), total_games=total)
    mine = pickle.load(open(path, "rb"))
    assert len(mine) == len(ref_games)

    def replay(game_info):                                   # view_best_games.py:193-213
        env = ChineseChess()
        env.reset()
        boards = [env.board.copy()]
        for board_state, move_probs, player in game_info["game_data"]:
            if move_probs:
                best = max(move_probs.items(), key=lambda x: x[1])[0]
                env.make_move(best)
                boards.append(env.board.copy())
        return boards

    for a, b in zip(mine, ref_games):
        assert set(a) == set(b) == {"timestamp", "total_games", "game_data", "winner", "moves", "type"}
        assert (a["total_games"], a["winner"], a["moves"], a["type"]) == (b["total_games"], b["winner"], b["moves"], b["type"])
        assert type(a["timestamp"]) is type(b["timestamp"]) and len(a["game_data"]) == len(b["game_data"])
        for (ba, pa, za), (bb, pb, zb) in zip(a["game_data"], b["game_data"]):
            assert ba.dtype == bb.dtype and ba.shape == bb.shape and np.array_equal(ba, bb)
            assert list(pa.keys()) == list(pb.keys())
            assert [struct.pack("<d", float(v)) for v in pa.values()] == [struct.pack("<d", float(v)) for v in pb.values()]
            assert type(next(iter(pa.values()))) is type(next(iter(pb.values())))
            assert struct.pack("<d", za) == struct.pack("<d", zb) and type(za) is type(zb)
        ra, rb = replay(a), replay(b)
        assert len(ra) == len(rb) and all(np.array_equal(x, y) for x, y in zip(ra, rb))
    # checkpoint structure
    st = json.load(open(os.path.join(golden_dir, "checkpoint_struct.json")))
    net = ChessNet()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    p = tmp_path / "models" / "latest.pt"
    formats.save_checkpoint(str(p), net, opt, total_games=st["total_games"], training_steps=st["training_steps"])
    ck = torch.load(str(p), map_location="cpu")
    assert sorted(ck.keys()) == st["keys"] and ck["total_games"] == st["total_games"] and ck["training_steps"] == st["training_steps"]
    assert {k: [list(v.shape), str(v.dtype)] for k, v in ck["model_state_dict"].items()} == st["model"]
    assert sorted(ck["optimizer_state_dict"].keys()) == st["optimizer_keys"]
    assert sorted(ck["optimizer_state_dict"]["param_groups"][0].keys()) == st["param_group_keys"]
    assert len(ck["optimizer_state_dict"]["param_groups"][0]["params"]) == st["n_param_ids"]
    # (the reference also writes models/model_<N>.pt when total_games % 1000 == 0: trainer.py:446-450)
    assert st["files"] == ["latest.pt", "model_1000.pt"]
    net2, meta = formats.load_checkpoint(str(p))
    assert meta["total_games"] == st["total_games"] and net2.num_blocks == 4


def test_interrupt_returns_the_games_already_finished(L, monkeypatch):
    """self_play.py:436-452: Ctrl-C during parallel_self_play raises InterruptedWithResults carrying the games that
    had finished.  Three S=50 games with the exact evaluator; seed 2 ends by checkmate at ply 33; the interrupt
    arrives at ply 40: exactly that game comes back, equal to the oracle's."""
    from chinesechessai_amd import engine as xe
    from chinesechessai_amd.chess_env import encode_move
    from chinesechessai_amd.engine import HashNetEvaluator
    from chinesechessai_amd.self_play import InterruptedWithResults, parallel_self_play
    from oracle import xq_oracle as xo
    calls = {"n": 0}
    real = xe.SelfPlayEngine.search

    def search(self, ev, **kw):
        calls["n"] += 1
        if calls["n"] == 41:
            raise KeyboardInterrupt
        return real(self, ev, **kw)

    monkeypatch.setattr(xe.SelfPlayEngine, "search", search)
    with pytest.raises(InterruptedWithResults) as ei:
        parallel_self_play(HashNetEvaluator(), 3, num_simulations=50, seeds=np.array([0, 2, 1], np.uint32))
    res = ei.value.results
    assert len(res) == 1
    gd, winner, reason = res[0]
    rc, og = xo.self_play_game(2, 50)
    assert winner == og.winner == 1 and reason == "将死黑方" and len(gd) == og.n_samples == 33
    for i, (board, pi, z) in enumerate(gd):
        k = og.s_nmoves[i]
        assert [encode_move(m) for m in pi.keys()] == list(og.s_moves[i][:k])
        assert struct.pack("<d", z) == struct.pack("<d", og.s_z[i])


def test_policy_fc_and_value_head_kernels_vs_torch(L):
    """csrc/xq_policy.hip through the C ABI against an fp32 torch evaluation of the same bf16 operands: the policy
    FC (both column sets: 2,304 = reachable, 8,256 = all 8,100 padded) and the value head, for row counts that
    exercise the tile tails (1, 37, 255, 256, 300, 4,097 rows; 256-row tiles, 16-row waves), nothing written past
    the last row, bit-identical results on repeated launches and for the same row inside batches of different
    sizes (the accumulation order does not depend on the launch), and loud rejection of shapes the kernel does not
    cover."""
    import torch
    from chinesechessai_amd import _lib
    from chinesechessai_amd.neural_network import ChessNet, InferenceNet
    st = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(5)
    net = ChessNet(num_blocks=1).eval().cuda()
    for mode, npol in (("reachable", 2304), ("all", 8256)):
        inet = InferenceNet(net, policy_columns=mode)
        assert inet.n_policy == npol and inet.pfw.shape == (npol, 2880)
        ref_rows = None
        for M in (4097, 1, 37, 255, 256, 300):
            g = torch.Generator(device="cuda").manual_seed(1)
            hp = (torch.rand(4097, 2880, device="cuda", generator=g) * (torch.rand(4097, 2880, device="cuda", generator=g) < 0.5)).bfloat16()[:M].contiguous()
            flat = torch.zeros(M * 720 + 64, dtype=torch.bfloat16, device="cuda")
            hv = flat[:M * 720].view(M, 720)
            hv.copy_((torch.rand(4097, 720, device="cuda", generator=g))[:M].bfloat16())
            out = torch.full((M + 1, npol), 7.0, dtype=torch.bfloat16, device="cuda")
            val = torch.full((M + 1,), 7.0, dtype=torch.bfloat16, device="cuda")
            for rep in range(2):
                _lib.check(L.xq_policy_fc_bf16(st, hp.data_ptr(), inet.pfw.data_ptr(), inet.hip_pfb.data_ptr(), out.data_ptr(), M, npol, 2880, None))
                _lib.check(L.xq_value_head_bf16(st, hv.data_ptr(), inet.hip_v1w.data_ptr(), inet.hip_v1b.data_ptr(),
                                                inet.hip_v2w.data_ptr(), inet.hip_v2b.data_ptr(), val.data_ptr(), M, None))
                torch.cuda.synchronize()
                if rep == 0:
                    first = (out.clone(), val.clone())
            assert torch.equal(out, first[0]) and torch.equal(val, first[1])                       # run to run
            assert (out[M] == 7.0).all() and val[M] == 7.0                                        # nothing past the last row
            ref = hp.float() @ inet.pfw.float().t() + inet.hip_pfb
            assert (out[:M].float() - ref).abs().max().item() <= 2 ** -8 * max(1.0, ref.abs().max().item())
            h1 = torch.relu(hv.float() @ inet.hip_v1w.float()[:, :720].t() + inet.hip_v1b)
            vref = torch.tanh(h1 @ inet.hip_v2w + inet.hip_v2b)
            assert (val[:M].float() - vref).abs().max().item() <= 2 ** -7
            if M == 4097:
                ref_rows = (out[:300].clone(), val[:300].clone())
            else:                                                                                 # same rows, other batch size
                k = min(M, 300)
                assert torch.equal(out[:k], ref_rows[0][:k]) and torch.equal(val[:k], ref_rows[1][:k]), (mode, M)
        assert L.xq_policy_fc_bf16(st, hp.data_ptr(), inet.pfw.data_ptr(), inet.hip_pfb.data_ptr(), out.data_ptr(), 4, npol - 1, 2880, None) == -1
        assert L.xq_policy_fc_bf16(st, hp.data_ptr(), inet.pfw.data_ptr(), inet.hip_pfb.data_ptr(), out.data_ptr(), 4, npol, 2870, None) == -1
        assert L.xq_policy_fc_bf16(st, None, inet.pfw.data_ptr(), inet.hip_pfb.data_ptr(), out.data_ptr(), 4, npol, 2880, None) == -1
    assert L.xq_value_head_bf16(st, None, None, None, None, None, None, 4, None) == -1


def test_root_eval_carry_is_result_identical(L):
    """xq_engine_set_root_eval_carry (automatic since round 3 wherever it is result-identical): the played child's network evaluation is carried over as the next root's
    instead of being computed a second time (the reference rebuilds its tree every ply and evaluates the root
    again, self_play.py:98).  Moves, root visit counts, z and outcomes must be bit-identical to the default path —
    with the exact evaluator against the oracle as well (seed 2 ends by checkmate at ply 33), with the bf16 network
    on the hand-written kernels, and under refill — while the evaluator is called (rounds - 1) times per ply after
    the first; and the option must refuse the combinations it cannot serve."""
    import torch
    from chinesechessai_amd import _lib, distributed as xd
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    from oracle import xq_oracle as xo

    class Counting:
        def __init__(self, ev):
            self.ev, self.calls, self.planes_format = ev, 0, ev.planes_format

        def bind(self, e): self.ev.bind(e)
        def planes_ptr(self): return self.ev.planes_ptr()

        def evaluate(self, e):
            self.calls += 1
            return self.ev.evaluate(e)

    def play(make_ev, G, S, carry, max_moves=70, seeds=None):
        ev = Counting(make_ev())
        eng = SelfPlayEngine(G, sims=S, planes_format=ev.planes_format, max_moves=max_moves)
        eng.set_root_eval_carry(bool(carry))            # (left alone the engine decides by itself: on, here)
        b = eng.play(ev, np.arange(G, dtype=np.uint32) if seeds is None else seeds)
        rows = eng.row_history()[0] if eng.row_compaction else None
        eng.close()
        return (b, ev.calls) if rows is None else (b, rows)

    # exact evaluator, whole games, vs the default path and vs the oracle
    seeds = np.array([2, 0, 1, 3, 7, 11], np.uint32)
    a, calls_a = play(HashNetEvaluator, 6, 50, False, seeds=seeds)
    b, calls_b = play(HashNetEvaluator, 6, 50, True, seeds=seeds)
    for k in ("chosen", "s_counts", "s_moves", "s_n", "winner", "reason", "n_plies", "n_samples", "error"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.s_z.view(np.int64), b.s_z.view(np.int64))
    rc, og = xo.self_play_game(2, 50)
    assert b.n_plies[0] == og.n_plies == 33 and list(og.t_move[:33]) == b.chosen[0, :33].tolist()
    plies = int(a.n_plies.max())
    assert calls_a == 7 * plies and calls_b == 6 * plies + 1, (calls_a, calls_b, plies)      # round 0 only at ply 0
    # the bf16 network
    torch.manual_seed(1)
    net = ChessNet(num_blocks=2).eval().cuda()
    # (leaf_dedupe=False, eval_cache=False: the row accounting below is the compaction's; tests/test_gpu_round3.py covers the
    # dedupe, tests/test_gpu_round5.py the evaluation cache - which would answer the roots the no-carry path evaluates again)
    a, ra = play(lambda: TorchNetEvaluator(net, leaf_dedupe=False, eval_cache=False), 96, 24, False, max_moves=14)
    b, rb = play(lambda: TorchNetEvaluator(net, leaf_dedupe=False, eval_cache=False), 96, 24, True, max_moves=14)
    assert np.array_equal(a.chosen, b.chosen) and np.array_equal(a.s_counts, b.s_counts)
    assert np.array_equal(a.s_z.view(np.int64), b.s_z.view(np.int64)) and int(b.error.sum()) == 0
    # the hand-written evaluator runs with row compaction: every round is launched, a carried root has no row in round 0
    assert len(ra) == len(rb) == 3 * 14 and (ra == 96).all()
    assert rb.reshape(14, 3)[1:, 0].tolist() == [0] * 13 and rb.sum() == 96 * (2 * 14 + 1)
    # refill: restarted slots get their round 0, everybody else skips it
    rs = np.array([2, 0, 1, 3, 2, 5, 2, 6, 7, 2], dtype=np.uint32)
    outs = []
    for carry in (False, True):
        eng = SelfPlayEngine(4, sims=50)
        eng.set_root_eval_carry(carry)
        rec_t = torch.zeros(len(rs) * 70 * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
        ev = Counting(HashNetEvaluator())
        out, n_plies = eng.play_refill(ev, rs, rec_t.data_ptr(), check_every=1)
        outs.append((out, rec_t.cpu().numpy().copy(), n_plies, ev.calls))
        eng.close()
    assert outs[0][2] == outs[1][2] == 140 and np.array_equal(outs[0][1], outs[1][1])
    assert all(np.array_equal(outs[0][0][k], outs[1][0][k]) for k in outs[0][0])
    assert outs[1][3] < outs[0][3] and outs[0][3] == 7 * 140
    # combinations the option does not serve
    eng = SelfPlayEngine(2, sims=16)
    eng.set_root_eval_carry(True)
    for fn in (lambda: eng.set_tree_reuse(True), lambda: eng.set_virtual_loss(True), lambda: eng.set_root_noise(0.3, 0.25)):
        with pytest.raises(_lib.XqError):
            fn()
    eng.close()
    eng = SelfPlayEngine(2, sims=16, opponent_mode=True)
    with pytest.raises(_lib.XqError):
        eng.set_root_eval_carry(True)
    eng.close()


def test_results_do_not_depend_on_the_sharding(L):
    """(e): games are sharded across ranks by contiguous index blocks with seeds base + g (distributed.game_seeds).  A
    game's result must not depend on which shard it lands in, on the shard's size or on its row in the evaluator
    batch — with the real bf16 network, not only with the exact evaluator: 96 games as one batch == the same games
    as shards of 64 + 32 and of 1 + 95, bit for bit (round 1 could not assert this: its library GEMM was not
    reproducible)."""
    import torch
    from chinesechessai_amd import distributed as xd
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet
    torch.manual_seed(2)
    net = ChessNet(num_blocks=2).eval().cuda()
    N, S, P = 96, 24, 10

    def play(seeds):
        ev = TorchNetEvaluator(net)
        eng = SelfPlayEngine(len(seeds), sims=S, planes_format=ev.planes_format, max_moves=P)
        b = eng.play(ev, seeds)
        eng.close()
        return b

    whole = play(xd.game_seeds(500, N, 0, 1))
    assert int(whole.error.sum()) == 0
    for cuts in ((0, 64, 96), (0, 1, 96)):
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            part = play((np.uint64(500) + np.arange(lo, hi, dtype=np.uint64)).astype(np.uint32))
            assert np.array_equal(part.chosen, whole.chosen[lo:hi]) and np.array_equal(part.s_counts, whole.s_counts[lo:hi])
            assert np.array_equal(part.s_z.view(np.int64), whole.s_z[lo:hi].view(np.int64))
    # and the shard arithmetic itself: the seeds of a 3-rank run are those of the single-rank run
    assert np.array_equal(np.concatenate([xd.game_seeds(500, N, r, 3) for r in range(3)]), xd.game_seeds(500, N, 0, 1))
