"""Policy targets from the device-resident replay ring (xq_replay_encode_policy_batch) and the fused legal-move
cross-entropy (xq_policy_loss_f32 / xq_policy_loss_grad_f32) on an MI355X, against the NumPy restatements of
tests/policy_reference.py (which tests/test_policy_targets_cpu.py holds against the package's host code)."""
import collections
import ctypes as C

import numpy as np
import pytest

from chinesechessai_amd import _lib
from chinesechessai_amd import distributed as xd
from chinesechessai_amd.chess_env import decode_move, encode_move
from tests import policy_reference as pr

pytestmark = pytest.mark.gpu

CAP = 40                                            # ring size: smaller than the first push, so the ring's head moves
UNREACHABLE = (0, 0, 9, 8)                          # corner to corner: no piece moves like that (no compact column)


# ---- the ring every target test samples: hand-made records through push_records, then one game through push() ----------
def _handmade(rng):
    from tests import wide_positions as wp
    recs = []
    side = 1
    for n in pr.N_MOVES:
        for kind in ("zeros", "single", "tie", "big"):
            moves = rng.choice(8100, n, replace=False)
            if kind == "zeros":
                counts = np.where(rng.random_sample(n) < 0.4, 0, rng.randint(1, 50, n))
                counts[n - 1] = 3
            elif kind == "single":
                counts = np.zeros(n, np.int64)
                counts[n // 2] = 17
            elif kind == "tie":
                counts = rng.randint(0, 20, n)
                counts[[n // 3, n - 1]] = 40                     # the first of the two must win at T < 0.01
            else:
                counts = rng.randint(0, 65536, n)
                counts[0] = 65535
            board = rng.randint(-7, 8, size=(10, 9)).astype(np.int8)
            recs.append(pr.make_record(board, moves, counts, float(rng.standard_normal()), player=side))
            side = -side
    # a real position with more than 64 legal moves (all of them reachable columns), black and red to move
    for name in ("w104", "lawful_both_black"):
        legal = wp.env_of(name).legal_moves()
        assert len(legal) > 64
        recs.append(pr.make_record(wp.board90(name).reshape(10, 9), legal, rng.randint(0, 30, len(legal)) + 1, 0.25,
                                   player=wp.entry(name)[4]))
    return recs


def _pushed_game(rng):
    game = []
    for k in (5, 1, 70):
        moves = [decode_move(int(m)) for m in rng.choice(8100, k, replace=False)]
        if k == 5:
            moves[2] = UNREACHABLE
        p = rng.random_sample(k)
        game.append((rng.randint(-7, 8, size=(10, 9)).astype(np.int8), dict(zip(moves, p / p.sum())), float(rng.standard_normal())))
    return game


@pytest.fixture(scope="module")
def ring():
    """(ReplayBuffer, the records it must hold oldest first).  12 filler records and the hand-made ones go through
    push_records in one push larger than the ring; three samples follow through push()."""
    import torch
    from chinesechessai_amd.replay import ReplayBuffer
    rng = np.random.RandomState(21)
    hand = _handmade(rng)
    filler = [pr.make_record(np.zeros((10, 9), np.int8), [100 + i], [1], 0.0) for i in range(12)]
    blocks = np.zeros((2, _lib.MAX_PLIES), dtype=xd.RECORD_DTYPE)
    blocks[0, :len(filler)] = np.array(filler, dtype=xd.RECORD_DTYPE)
    blocks[1, :len(hand)] = np.array(hand, dtype=xd.RECORD_DTYPE)
    assert len(hand) <= _lib.MAX_PLIES and len(filler) + len(hand) > CAP
    buf = ReplayBuffer(max_size=CAP)
    want = collections.deque(maxlen=CAP)
    t = torch.from_numpy(np.frombuffer(blocks.tobytes(), dtype=np.uint8).copy()).cuda()
    assert buf.push_records(t, 2) == len(filler) + len(hand)
    want.extend(filler + hand)
    game = _pushed_game(rng)
    assert buf.push(game) == len(game)
    for board, probs, z in game:                                  # the record push() forms (replay.py)
        counts = [int(round(min(max(float(p), 0.0), 1.0) * 65535)) for p in probs.values()]
        want.append(pr.make_record(board, [encode_move(m) for m in probs], counts, z, player=0))
    want = np.array(list(want), dtype=xd.RECORD_DTYPE)
    back = np.zeros(CAP, dtype=xd.RECORD_DTYPE)
    idx = np.arange(CAP, dtype=np.int64)
    buf._chk(buf.L.xq_replay_read_records(buf.h, C.c_void_p(buf._stream()), _lib.ptr(idx), CAP, _lib.ptr(back)))
    assert back.tobytes() == want.tobytes()                       # the ring holds what this file thinks it holds
    assert len(buf) == CAP and {int(n) for n in want["n_moves"]} >= set(pr.N_MOVES)
    assert {int(p) for p in want["player"]} == {-1, 0, 1}
    yield buf, want
    buf.close()


def _indices(batch, salt):
    rng = np.random.RandomState(100 + batch + salt)
    if batch >= CAP:
        return np.concatenate([np.arange(CAP), rng.randint(0, CAP, batch - CAP)]).astype(np.int64)   # every record, some twice
    return rng.choice(CAP, batch, replace=False).astype(np.int64)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)                                           # (pi >= 0: the bit patterns are ordered)


@pytest.mark.parametrize("batch", [1, 3, 65])
@pytest.mark.parametrize("temperature", [1.0, 0.5, 0.001, 0.7])
def test_pi_and_columns_equal_record_to_sample(ring, batch, temperature):
    """pi bit for bit float32(record_to_sample) at the reference's two training temperatures (trainer.py:166) and in the
    argmax branch; within one float32 ulp at T = 0.7, where neither side's pow is correctly rounded; cols = moves."""
    buf, want = ring
    idx = _indices(batch, 0)
    states, tv, tg = buf.sample_policy_tensors(batch, indices=idx, temperature=temperature)
    assert states.shape == (batch, 15, 10, 9) and tv.shape == (batch, 1)
    assert tg.cols.shape == tg.pi.shape == (batch, 128) and tg.n_moves.shape == (batch,)
    cols, pi, nm, tv = tg.cols.cpu().numpy(), tg.pi.cpu().numpy(), tg.n_moves.cpu().numpy(), tv.cpu().numpy()
    worst, ties = 0, 0
    for b, i in enumerate(idx):
        rec = want[i]
        n = int(rec["n_moves"])
        _, probs, z = xd.record_to_sample(rec, temperature)
        ref = np.zeros(128, np.float32)
        ref[:n] = np.float32(np.array(list(probs.values()), np.float64))
        assert nm[b] == n and np.array_equal(cols[b, :n], rec["moves"][:n].astype(np.int32)) and (cols[b, n:] == -1).all(), (b, i)
        assert (pi[b, n:] == 0).all(), (b, i)
        if temperature == 0.7:
            worst = max(worst, int(_ulps(pi[b], ref).max()))
            assert _ulps(pi[b], ref).max() <= 1, (b, i)
        else:
            assert pi[b].tobytes() == ref.tobytes(), (b, i, temperature)
        assert np.float32(z) == tv[b, 0]
        if temperature < 0.01:                                     # np.argmax: the first maximum
            c = rec["counts"][:n]
            first = int(np.flatnonzero(c == c.max())[0])
            assert int(np.argmax(pi[b])) == first and pi[b, first] == 1 and pi[b].sum() == 1, (b, i)
            ties += int((c == c.max()).sum() > 1)
    if temperature == 0.7:
        print("T=0.7 B=%d: largest difference to float32(record_to_sample) = %d ulp" % (batch, worst))
    if temperature < 0.01 and batch >= CAP:
        assert ties >= 5                                           # the records built with a tie for the maximum
    # the buffer's own temperature is the default
    old, buf.temperature = buf.temperature, temperature
    try:
        _, _, tg2 = buf.sample_policy_tensors(batch, indices=idx)
    finally:
        buf.temperature = old
    assert tg2.pi.cpu().numpy().tobytes() == pi.tobytes()


def test_states_and_values_equal_sample_tensors(ring):
    import torch
    buf, want = ring
    for batch in (1, 3, 65):
        idx = _indices(batch, 1)
        s0, t0 = buf.sample_tensors(batch, indices=idx)
        s1, t1, _ = buf.sample_policy_tensors(batch, indices=idx)
        s2, t2, _ = buf.sample_policy_tensors(batch, indices=idx, mirror=np.zeros(batch, bool), player_plane="red")
        for s, t in ((s1, t1), (s2, t2)):
            assert s.cpu().numpy().tobytes() == s0.cpu().numpy().tobytes() and t.cpu().numpy().tobytes() == t0.cpu().numpy().tobytes()
    # without indices: the same single draw from NumPy's global stream as sample_tensors (trainer.py:37)
    np.random.seed(5)
    s0, t0 = buf.sample_tensors(7)
    np.random.seed(5)
    s1, t1, tg = buf.sample_policy_tensors(7)
    np.random.seed(5)
    idx = np.random.choice(CAP, 7, replace=False)
    assert torch.equal(s0, s1) and torch.equal(t0, t1)
    assert np.array_equal(tg.n_moves.cpu().numpy(), want["n_moves"][idx].astype(np.int32))
    with pytest.raises(_lib.XqError, match="out of range"):
        buf.sample_policy_tensors(2, indices=np.array([0, CAP]))
    with pytest.raises(_lib.XqError, match="out of range"):
        buf.sample_policy_tensors(1, indices=np.array([-1]))
    with pytest.raises(ValueError):
        buf.sample_policy_tensors(1, indices=np.array([0]), player_plane="black")
    # the powers of a temperature other than 1 come from the host (the device's pow is not NumPy's): refused without them
    one = np.zeros(1, np.int64)
    out = [C.c_void_p(x.data_ptr()) for x in (s1, t1, tg.cols, tg.pi, tg.n_moves)]
    assert buf.L.xq_replay_encode_policy_batch(buf.h, None, _lib.ptr(one), 1, None, 0, 0.7, None, 0, None, *out) == -1
    assert b"table" in buf.L.xq_replay_last_error()
    assert buf.L.xq_replay_encode_policy_batch(buf.h, None, _lib.ptr(one), 1, None, 2, 1.0, None, 0, None, *out) == -1
    assert buf.L.xq_replay_encode_policy_batch(buf.h, None, _lib.ptr(one), 1, None, 0, 1.0, None, 0, None, *out) == 0
    torch.cuda.synchronize()


def test_compact_column_map(ring):
    import torch
    from chinesechessai_amd.neural_network import reachable_policy_columns
    buf, want = ring
    _, cmap = reachable_policy_columns()
    idx = np.arange(CAP, dtype=np.int64)
    dev_map = torch.from_numpy(cmap.astype(np.int32)).cuda()
    for cm in (cmap, dev_map):                                    # the host table (int16) and a device int32 tensor
        _, _, tg = buf.sample_policy_tensors(CAP, indices=idx, column_map=cm)
        cols = tg.cols.cpu().numpy()
        for b in range(CAP):
            n = int(want[b]["n_moves"])
            assert np.array_equal(cols[b, :n], cmap[want[b]["moves"][:n].astype(np.int64)].astype(np.int32)), b
            assert (cols[b, n:] == -1).all(), b
    # the pushed game's hand-placed unreachable move has no column; the real wide positions have one for every move
    first_pushed = CAP - 3
    assert want[first_pushed]["moves"][2] == encode_move(UNREACHABLE) and cols[first_pushed, 2] == -1
    wide = [b for b in range(CAP) if want[b]["z"] == 0.25]
    assert len(wide) == 2 and all((cols[b, :int(want[b]["n_moves"])] >= 0).all() and want[b]["n_moves"] > 64 for b in wide)
    with pytest.raises(ValueError):
        buf.sample_policy_tensors(1, indices=idx[:1], column_map=cmap[:100])


def test_player_plane_of_the_record(ring):
    from chinesechessai_amd.neural_network import ChessNet
    buf, want = ring
    idx = np.arange(CAP, dtype=np.int64)
    s_red, _, _ = buf.sample_policy_tensors(CAP, indices=idx)
    s_rec, _, _ = buf.sample_policy_tensors(CAP, indices=idx, player_plane="record")
    s_red, s_rec = s_red.cpu().numpy(), s_rec.cpu().numpy()
    seen = set()
    for b in range(CAP):
        board, player = xd.unpack_board(want[b]["board"]), int(want[b]["player"])
        assert s_red[b].tobytes() == ChessNet.encode_board(board, 1).tobytes(), b
        # a record without a side (push() writes player 0) is nobody's move: plane 14 is zero, as encode_board(board, 0)
        assert s_rec[b].tobytes() == ChessNet.encode_board(board, player).tobytes(), b
        seen.add((player, float(s_rec[b, 14, 0, 0])))
    assert seen == {(1, 1.0), (-1, 0.0), (0, 0.0)}


def test_mirrored_samples(ring):
    from chinesechessai_amd.neural_network import ChessNet, reachable_policy_columns
    buf, want = ring
    _, cmap = reachable_policy_columns()
    idx = np.arange(CAP, dtype=np.int64)
    flags = np.random.RandomState(3).random_sample(CAP) < 0.5
    flags[-6:] = True                                             # the wide positions and the pushed game among them
    for cm in (None, cmap):
        s, tv, tg = buf.sample_policy_tensors(CAP, indices=idx, mirror=flags, column_map=cm, player_plane="record")
        s0, tv0, tg0 = buf.sample_policy_tensors(CAP, indices=idx, column_map=cm, player_plane="record")
        s, cols = s.cpu().numpy(), tg.cols.cpu().numpy()
        assert tg.pi.cpu().numpy().tobytes() == tg0.pi.cpu().numpy().tobytes()            # pi does not move
        assert tv.cpu().numpy().tobytes() == tv0.cpu().numpy().tobytes()
        assert np.array_equal(tg.n_moves.cpu().numpy(), tg0.n_moves.cpu().numpy())
        for b in range(CAP):
            rec = pr.mirror_record(want[b]) if flags[b] else want[b]
            assert s[b].tobytes() == ChessNet.encode_board(xd.unpack_board(rec["board"]), int(rec["player"])).tobytes(), b
            assert np.array_equal(cols[b], pr.target_of_record(rec, 1.0, column_map=cm)[0]), b
            if flags[b] and cm is None:
                assert np.array_equal(cols[b], pr.target_of_record(want[b], 1.0, mirror=True)[0]), b
    # one flag for the whole batch
    s1, _, tg1 = buf.sample_policy_tensors(3, indices=idx[:3], mirror=True)
    s2, _, tg2 = buf.sample_policy_tensors(3, indices=idx[:3], mirror=np.ones(3, bool))
    assert s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes() and np.array_equal(tg1.cols.cpu().numpy(), tg2.cols.cpu().numpy())


def test_targets_of_a_played_game_equal_game_data():
    """SelfPlayEngine -> pack_samples -> push_records -> sample_policy_tensors: cols and pi are the move_probs dicts of
    GameBatch.game_data (what the reference's self_play_game returns), states the real side to move's encoding"""
    import torch
    from chinesechessai_amd.engine import HashNetEvaluator, SelfPlayEngine
    from chinesechessai_amd.neural_network import ChessNet
    from chinesechessai_amd.replay import ReplayBuffer
    for T in (1.0, 0.5):
        eng = SelfPlayEngine(3, sims=24, max_moves=6, temperature=T)
        bt = eng.play(HashNetEvaluator(), np.array([7, 8, 9], np.uint32))
        rec_t = torch.zeros(3 * _lib.MAX_PLIES * xd.RECORD_BYTES, dtype=torch.uint8, device="cuda")
        eng.pack_samples(rec_t.data_ptr())
        eng.close()
        data = [s for g in range(3) for s in bt.game_data(g)]
        sides = [int(bt.s_player[g, i]) for g in range(3) for i in range(int(bt.n_samples[g]))]
        buf = ReplayBuffer(max_size=64, temperature=T)
        assert buf.push_records(rec_t, 3) == len(data) == len(buf)
        states, tv, tg = buf.sample_policy_tensors(len(data), indices=np.arange(len(data)), player_plane="record")
        buf.close()
        states, tv, cols, pi, nm = (x.cpu().numpy() for x in (states, tv, tg.cols, tg.pi, tg.n_moves))
        for b, (board, probs, z) in enumerate(data):
            n = len(probs)
            assert nm[b] == n and [decode_move(int(c)) for c in cols[b, :n]] == list(probs.keys()), b
            assert pi[b, :n].tobytes() == np.float32(np.array(list(probs.values()))).tobytes() and not pi[b, n:].any(), b
            assert tv[b, 0] == np.float32(z) and states[b].tobytes() == ChessNet.encode_board(board, sides[b]).tobytes(), b


# ---- loss and gradient ----------------------------------------------------------------------------------------------------
LOSS_N = (0,) + pr.N_MOVES


def _loss_cases(n_cols, seed):
    """logits float32 [B][n_cols], cols, pi float32, n_moves: one row per n of LOSS_N with randn logits, the same again
    scaled to +-80, and one row with a -1 column.  Row k's legal columns include 0, n_cols - 1 and two neighbours inside one
    16-byte group whenever it has that many slots."""
    rng = np.random.RandomState(seed)
    rows = []
    for scale in (1.0, 80.0):
        for n in LOSS_N:
            rows.append((n, scale, False))
    rows.append((65, 1.0, True))
    B = len(rows)
    logits = rng.standard_normal((B, n_cols)).astype(np.float32)
    cols = np.full((B, 128), -1, np.int32)
    pi = np.zeros((B, 128), np.float32)
    nm = np.zeros(B, np.int32)
    for b, (n, scale, masked) in enumerate(rows):
        nm[b] = n
        if scale != 1.0:
            logits[b] = np.where(rng.random_sample(n_cols) < 0.5, 80.0, -80.0) + logits[b]
        fixed = [0, n_cols - 1, 1000, 1001][:n]
        rest = rng.choice(np.setdiff1d(np.arange(1, n_cols - 1), [1000, 1001]), n - len(fixed), replace=False)
        c = np.concatenate([fixed, rest]).astype(np.int32)
        rng.shuffle(c)
        cols[b, :n] = c
        p = rng.random_sample(n) * (rng.random_sample(n) < 0.7)
        if n:
            p[rng.randint(n)] += 0.1
            pi[b, :n] = np.float32(p / p.sum())
        if masked:
            cols[b, 5] = -1                                        # a slot with probability mass and no column
            cols[b, 64] = -1
        # garbage beyond n_moves must not be read
        cols[b, n:] = rng.randint(-5, n_cols, 128 - n) if b % 2 else -1
        pi[b, n:] = 0.5 if b % 2 else 0.0
    return logits, cols, pi, nm


def _run_loss(logits_t, cols_t, pi_t, nm_t, stride=None):
    import torch
    L = _lib.lib()
    B, n_cols = logits_t.shape if stride is None else (logits_t.shape[0], stride[1])
    loss = torch.full((B,), float("nan"), device="cuda")
    resid = torch.full((B, 128), float("nan"), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    rc = L.xq_policy_loss_f32(C.c_void_p(s), C.c_void_p(logits_t.data_ptr()), logits_t.stride(0) if stride is None else stride[0],
                              n_cols, C.c_void_p(cols_t.data_ptr()), C.c_void_p(pi_t.data_ptr()), C.c_void_p(nm_t.data_ptr()), B,
                              C.c_void_p(loss.data_ptr()), C.c_void_p(resid.data_ptr()))
    assert rc == 0
    return loss, resid


def _run_grad(resid_t, cols_t, nm_t, n_cols, row_stride, scale_dev=None, scale_host=1.0, offset=0):
    """dense gradient into a NaN-filled buffer [B][row_stride] starting `offset` floats into an allocation"""
    import torch
    L = _lib.lib()
    B = resid_t.shape[0]
    store = torch.full((B * row_stride + offset,), float("nan"), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    rc = L.xq_policy_loss_grad_f32(C.c_void_p(s), C.c_void_p(resid_t.data_ptr()), C.c_void_p(cols_t.data_ptr()),
                                   C.c_void_p(nm_t.data_ptr()), C.c_void_p(scale_dev.data_ptr()) if scale_dev is not None else None,
                                   scale_host, B, C.c_void_p(store.data_ptr() + 4 * offset), row_stride, n_cols)
    assert rc == 0
    torch.cuda.synchronize()
    return store[offset:].view(B, row_stride).cpu().numpy()


@pytest.fixture(scope="module")
def loss_runs():
    """per n_cols: inputs, the device's loss / resid / dense gradient (scale 1) and the float64 and float32 restatements"""
    import torch
    out = {}
    for n_cols in (8100, 2304):
        logits, cols, pi, nm = _loss_cases(n_cols, 31 + n_cols)
        lt, ct, pt, nt = (torch.from_numpy(x).cuda() for x in (logits, cols, pi, nm))
        loss, resid = _run_loss(lt, ct, pt, nt)
        grad = _run_grad(resid, ct, nt, n_cols, n_cols)
        usable = np.where(cols >= n_cols, -1, cols)                # (the garbage beyond n_moves is cut by n_moves anyway)
        ref64 = [pr.loss_of_row(logits[b], usable[b], pi[b], int(nm[b]), np.float64) for b in range(len(nm))]
        ref32 = [pr.loss_of_row(logits[b], usable[b], pi[b], int(nm[b]), np.float32) for b in range(len(nm))]
        out[n_cols] = dict(logits=logits, cols=cols, pi=pi, nm=nm, t=(lt, ct, pt, nt), loss=loss.cpu().numpy(),
                           resid=resid.cpu().numpy(), resid_t=resid, grad=grad, ref64=ref64, ref32=ref32)
    return out


def test_loss_residual_and_gradient_against_float64(loss_runs):
    """The bound is NumPy's own float32 arithmetic on the same inputs (as for the legal-logit softmax):
    the device's largest error against float64 may be at most twice NumPy-float32's largest error, over the whole case
    set, for the loss and for the gradient elements alike."""
    err = {"loss": [0.0, 0.0], "grad": [0.0, 0.0]}
    for n_cols, r in loss_runs.items():
        assert not np.isnan(r["loss"]).any() and not np.isnan(r["resid"]).any()
        assert not np.isnan(r["grad"]).any(), "an element of the gradient was never stored"
        for b in range(len(r["nm"])):
            l64, r64, g64 = r["ref64"][b]
            l32, r32, g32 = r["ref32"][b]
            n = int(r["nm"][b])
            err["loss"][0] = max(err["loss"][0], abs(float(r["loss"][b]) - l64))
            err["loss"][1] = max(err["loss"][1], abs(float(l32) - l64))
            err["grad"][0] = max(err["grad"][0], np.abs(r["grad"][b].astype(np.float64) - g64).max(),
                                 np.abs(r["resid"][b].astype(np.float64) - r64).max())
            err["grad"][1] = max(err["grad"][1], np.abs(g32.astype(np.float64) - g64).max())
            # the dense gradient is the residual at the legal columns and exactly 0.0 everywhere else
            legal = r["cols"][b, :n]
            legal = legal[legal >= 0]
            off = np.ones(n_cols, bool)
            off[legal] = False
            assert (r["grad"][b][off].view(np.int32) == 0).all(), (n_cols, b)          # +0.0, not merely == 0
            use = np.flatnonzero(r["cols"][b, :n] >= 0)
            assert r["grad"][b][r["cols"][b, use]].tobytes() == r["resid"][b, use].tobytes(), (n_cols, b)
            dead = np.setdiff1d(np.arange(128), use)
            assert (r["resid"][b, dead] == 0).all(), (n_cols, b)
            if len(use) == 0:
                assert r["loss"][b] == 0 and not r["resid"][b].any() and not r["grad"][b].any()
    print("largest error against float64 (device, NumPy float32): loss %.3e %.3e, gradient %.3e %.3e"
          % (err["loss"][0], err["loss"][1], err["grad"][0], err["grad"][1]))
    assert err["loss"][1] > 0 and err["grad"][1] > 0
    assert err["loss"][0] <= 2 * err["loss"][1], err
    assert err["grad"][0] <= 2 * err["grad"][1], err


def test_zero_probability_terms_and_masked_columns(loss_runs):
    """pi == 0 contributes exactly 0 even where log p underflows (+-80 rows); a slot with column -1 takes part in nothing
    although it carries probability mass"""
    for n_cols, r in loss_runs.items():
        assert np.isfinite(r["loss"]).all()
        b = len(r["nm"]) - 1                                       # the masked row
        assert r["cols"][b, 5] == -1 and r["pi"][b, 5] >= 0 and r["resid"][b, 5] == 0 and r["resid"][b, 64] == 0
        use = np.flatnonzero(r["cols"][b, :65] >= 0)
        p = r["resid"][b, use].astype(np.float64) + r["pi"][b, use]
        assert abs(p.sum() - 1) < 1e-5                             # the softmax runs over the usable slots alone


def test_gradient_scale_and_row_stride(loss_runs):
    """scale per row from device memory or one host float; a stride that breaks 16-byte row alignment takes the 4-byte
    stores and gives the same bits; nothing beyond n_cols is touched"""
    import torch
    for n_cols, r in loss_runs.items():
        lt, ct, pt, nt = r["t"]
        B = len(r["nm"])
        scale = np.random.RandomState(4).standard_normal(B).astype(np.float32)
        g = _run_grad(r["resid_t"], ct, nt, n_cols, n_cols, scale_dev=torch.from_numpy(scale).cuda())
        want = np.zeros((B, n_cols), np.float32)
        for b in range(B):
            for i in range(int(r["nm"][b])):
                c = r["cols"][b, i]
                if c >= 0:
                    want[b, c] = np.float32(scale[b] * r["resid"][b, i])
        assert np.array_equal(g, want), n_cols                     # (NaN, a value never stored, equals nothing)
        g = _run_grad(r["resid_t"], ct, nt, n_cols, n_cols, scale_host=-0.5)
        assert np.array_equal(g, np.float32(-0.5) * r["grad"]) and not np.isnan(g).any()
        for stride, offset in ((n_cols + 1, 0), (n_cols + 3, 0), (n_cols + 4, 0), (n_cols, 1)):
            g = _run_grad(r["resid_t"], ct, nt, n_cols, stride, offset=offset)
            assert g[:, :n_cols].tobytes() == r["grad"].tobytes(), (n_cols, stride, offset)
            assert np.isnan(g[:, n_cols:]).all(), (n_cols, stride, offset)
        # a row length that is no multiple of 4 behind an aligned stride: 16-byte stores and a tail of two floats; a
        # column at or beyond the row length is as unusable in the backward pass as it is in the forward pass
        g = _run_grad(r["resid_t"], ct, nt, n_cols - 2, n_cols)
        assert g[:, :n_cols - 2].tobytes() == r["grad"][:, :n_cols - 2].tobytes() and np.isnan(g[:, n_cols - 2:]).all()
        # the forward reads rows at a stride too
        wide = torch.full((B, n_cols + 5), float("nan"), device="cuda")
        wide[:, :n_cols] = lt
        loss, resid = _run_loss(wide, ct, pt, nt, stride=(n_cols + 5, n_cols))
        assert loss.cpu().numpy().tobytes() == r["loss"].tobytes() and resid.cpu().numpy().tobytes() == r["resid"].tobytes()


def test_rows_do_not_depend_on_batch_or_order(loss_runs):
    import torch
    for n_cols, r in loss_runs.items():
        lt, ct, pt, nt = r["t"]
        loss, resid = _run_loss(lt, ct, pt, nt)
        assert loss.cpu().numpy().tobytes() == r["loss"].tobytes() and resid.cpu().numpy().tobytes() == r["resid"].tobytes()
        perm = torch.from_numpy(np.random.RandomState(6).permutation(len(r["nm"]))[:11]).cuda()
        loss, resid = _run_loss(lt[perm].contiguous(), ct[perm].contiguous(), pt[perm].contiguous(), nt[perm].contiguous())
        p = perm.cpu().numpy()
        assert loss.cpu().numpy().tobytes() == r["loss"][p].tobytes() and resid.cpu().numpy().tobytes() == r["resid"][p].tobytes()
        g = _run_grad(resid, ct[perm].contiguous(), nt[perm].contiguous(), n_cols, n_cols)
        assert g.tobytes() == r["grad"][p].tobytes()


def _torch_reference(logits64, cols, pi, nm, reduction, upstream=None):
    """gather -> log_softmax -> -sum pi log p in float64 on the CPU, differentiated by torch autograd"""
    import torch
    x = torch.tensor(logits64, dtype=torch.float64, requires_grad=True)
    rows = []
    for b in range(len(nm)):
        use = [i for i in range(int(nm[b])) if cols[b, i] >= 0]
        if not use:
            rows.append(x[b, 0] * 0)
            continue
        lp = torch.log_softmax(x[b, torch.tensor(cols[b, use].astype(np.int64))], dim=0)
        t = torch.tensor(pi[b, use].astype(np.float64))
        rows.append(-(t[t != 0] * lp[t != 0]).sum())
    rows = torch.stack(rows)
    if reduction == "none":
        rows.backward(torch.tensor(upstream, dtype=torch.float64))
        return rows.detach().numpy(), x.grad.numpy()
    out = rows.mean() if reduction == "mean" else rows.sum()
    out.backward()
    return out.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_policy_loss_autograd(loss_runs, reduction):
    """training.policy_loss(...).backward() against torch autograd of the float64 restatement on the rows with randn
    logits.  Tolerances from the arithmetic, eps = 2**-24 (half a float32 ulp, relative), D = the largest spread of a
    row's legal logits, M = D + log(128) < D + 5 the largest |x - max - log sum|:
      gradient: exp's argument x - max is off by D eps, expf by 2 eps, the 8-level sum by 9 eps, division, subtraction
        of pi and the product with the scale by eps each: |g - g64| <= (D + 14) eps |scale| (p <= 1).
      row loss: x - max D eps; log of a sum that is off by 9 eps relative, logf itself 2 ulp of at most 5: 29 eps;
        the difference, the product with pi and the 8-level sum of the terms (sum pi = 1, partial sums <= M): 10 M eps:
        |l - l64| <= (11 D + 80) eps.
      reduction over B rows in float32, any order: B eps times the largest partial sum (B M for "sum", and "mean"
        divides by B)."""
    import torch
    from chinesechessai_amd import training
    from chinesechessai_amd.replay import PolicyTarget
    r = loss_runs[2304]
    keep = np.arange(len(LOSS_N))                                  # the randn rows
    logits, cols, pi, nm = (r[k][keep] for k in ("logits", "cols", "pi", "nm"))
    B = len(keep)
    cols = np.where(np.arange(128)[None, :] < nm[:, None], cols, -1).astype(np.int32)
    x = torch.from_numpy(logits).cuda().requires_grad_(True)
    target = PolicyTarget(torch.from_numpy(cols).cuda(), torch.from_numpy(pi).cuda(), torch.from_numpy(nm).cuda())
    upstream = np.random.RandomState(8).standard_normal(B).astype(np.float32) * 3
    out = training.policy_loss(x, target, reduction=reduction)
    if reduction == "none":
        assert out.shape == (B,)
        out.backward(torch.from_numpy(upstream).cuda())
        row_scale = np.abs(upstream).astype(np.float64)
    else:
        assert out.dim() == 0
        out.backward()
        row_scale = np.full(B, 1.0 / B if reduction == "mean" else 1.0)
    ref_out, ref_grad = _torch_reference(logits.astype(np.float64), cols, pi, nm, reduction, upstream)
    D = max(float(np.ptp(logits[b, cols[b, :nm[b]]])) for b in range(B) if nm[b])
    eps = 2.0 ** -24
    got = x.grad.cpu().numpy().astype(np.float64)
    assert (np.abs(got - ref_grad).max(axis=1) <= (D + 14) * eps * row_scale).all()
    assert not got[ref_grad == 0].any()
    row_tol, M = (11 * D + 80) * eps, D + 5
    loss_tol = {"none": row_tol, "mean": row_tol + B * M * eps, "sum": B * row_tol + B * B * M * eps}[reduction]
    assert np.abs(out.detach().cpu().numpy().astype(np.float64) - ref_out).max() <= loss_tol
    assert x.grad.shape == x.shape and x.grad.is_contiguous()


def test_python_layer_refuses_what_the_kernels_do_not_cover(loss_runs):
    import torch
    from chinesechessai_amd import training
    from chinesechessai_amd.replay import PolicyTarget
    r = loss_runs[2304]
    lt, ct, pt, nt = r["t"]
    target = PolicyTarget(ct, pt, nt)
    training.policy_loss(lt, target)
    wide = torch.zeros((lt.shape[0], 2400), device="cuda")
    for bad in (wide[:, :2304],                                    # a row stride that is not the row length
                lt.double(), lt.half(), lt.cpu(), lt[0], lt.t()):
        with pytest.raises(ValueError):
            training.policy_loss(bad, target)
    for bad in (PolicyTarget(ct[:3], pt, nt), PolicyTarget(ct.long(), pt, nt), PolicyTarget(ct, pt.double(), nt),
                PolicyTarget(ct, pt, nt.cpu()), PolicyTarget(ct[:, :64], pt[:, :64], nt)):
        with pytest.raises(ValueError):
            training.policy_loss(lt, bad)
    with pytest.raises(ValueError):
        training.policy_loss(lt, target, reduction="batchmean")


def test_one_step_trains_the_policy_head(ring):
    """What the feature adds: one optimizer step of training.loss moves policy_fc.weight; the reference's value-only
    loss (trainer.py:327-331) leaves it where it was."""
    import torch
    from chinesechessai_amd import training
    from chinesechessai_amd.neural_network import ChessNet
    buf, _ = ring
    torch.manual_seed(2)
    states, tv, target = buf.sample_policy_tensors(8, indices=np.arange(CAP - 8, CAP), player_plane="record")
    net = ChessNet(num_channels=16, num_blocks=2).cuda().train()
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    w0 = net.policy_fc.weight.detach().clone()
    v0 = net.value_fc2.weight.detach().clone()
    opt.zero_grad()
    logits, value = net(states)
    torch.nn.MSELoss()(value, tv).backward()                       # trainer.py:327-331
    opt.step()
    assert torch.equal(net.policy_fc.weight, w0) and not torch.equal(net.value_fc2.weight, v0)
    opt.zero_grad(set_to_none=True)
    total, value_loss, p_loss = training.loss(net, states, tv, target)
    assert total.dim() == value_loss.dim() == p_loss.dim() == 0 and p_loss.item() > 0
    assert total.item() == pytest.approx(value_loss.item() + p_loss.item(), rel=1e-6)
    total.backward()
    g = net.policy_fc.weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
    opt.step()
    assert not torch.equal(net.policy_fc.weight, w0)
    total, value_loss, _ = training.loss(net, states, tv, target, policy_weight=0.0)
    assert total.item() == value_loss.item()
