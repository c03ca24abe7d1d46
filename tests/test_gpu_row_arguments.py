"""GPU tests (`-m gpu`, through the C ABI) of the row arguments of the three evaluator kernels - xq_tower_nhwc_bf16
(row_src, n_rows), xq_policy_fc_bf16 (n_rows) and xq_value_head_bf16 (n_rows) - at small, ragged counts: 0, 1, one either
side of every tile edge, and a count larger than the launch's row count (clamped).

Method: every comparison is bit for bit against the SAME kernel's plain launch (no row_src / n_rows) on clean inputs;
inputs the launch must not read are poisoned (NaN - for the value head, whose 16 values behind each row meet zero weights,
the largest finite bf16 and finite garbage), outputs it must not write hold a sentinel.  No index in any array is out of
range: the poison is in the data, never in an address.  Each FC kernel is pinned once to a float64 reference with an
a-priori error bound computed from the operands (no measured constant)."""
import pytest

pytestmark = pytest.mark.gpu

SENT16 = 0x7FC1                         # int16 view of the output sentinel: a NaN pattern no kernel writes
NAN16 = 0x7FC0                          # bf16 quiet NaN
MAXF16 = 0x7F7F                         # the largest finite bf16 (3.39e38)


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


def _count(n):
    import torch
    return torch.tensor([n], device="cuda", dtype=torch.int32)


def _i16(t):
    import torch
    return t.view(torch.int16)


# ------------------------------------------------------------------------------------------------ trunk
TRUNK_G, TRUNK_PLANE_ROWS, TRUNK_NAN_ROW = 9, 12, 9
TRUNK_ROW_SRC = (3, 3, 7, 0, 11, 7, 5, 2, 3)            # not a permutation: repeats, rows 1, 4, 6, 8, 9, 10 never named


@pytest.fixture(scope="module")
def trunk_setup(L):
    import torch
    from chinesechessai_amd.neural_network import ChessNet, InferenceNet
    torch.manual_seed(77)
    net = ChessNet(num_blocks=1).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    inet = InferenceNet(net.cuda())
    g = torch.Generator(device="cuda").manual_seed(8)
    R = TRUNK_PLANE_ROWS
    code = torch.randint(0, 40, (R, 10, 9), device="cuda", generator=g)
    planes = torch.zeros(R, 10, 9, 16, device="cuda", dtype=torch.bfloat16)
    for c in range(14):
        planes[..., c] = (code == c + 1).to(torch.bfloat16)
    planes[..., 14] = (torch.arange(R, device="cuda") % 2).to(torch.bfloat16).view(R, 1, 1).expand(R, 10, 9)
    return inet, planes


def _trunk(L, inet, variant, planes, n_boards, out_rows, row_src=None, n_rows=None):
    import torch
    from chinesechessai_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    P = torch.full((out_rows, 2880), SENT16, device="cuda", dtype=torch.int16)
    V = torch.full((out_rows, 720), SENT16, device="cuda", dtype=torch.int16)
    L.xq_tower_set_variant(variant)
    try:
        _lib.check(L.xq_tower_nhwc_bf16(st, planes.data_ptr(), inet.hip_w[0].data_ptr(), inet.hip_wt.data_ptr(),
                                        inet.hip_bt.data_ptr(), inet.hip_hw.data_ptr(), inet.hip_hb.data_ptr(),
                                        P.data_ptr(), V.data_ptr(), n_boards, 1,
                                        None if row_src is None else row_src.data_ptr(),
                                        None if n_rows is None else n_rows.data_ptr()))
        torch.cuda.synchronize()
    finally:
        L.xq_tower_set_variant(-1)
    return P, V


@pytest.mark.parametrize("variant", (36, 39, 60, -1))
def test_trunk_row_map_and_count_at_small_ragged_counts(L, trunk_setup, variant):
    """xq_tower_nhwc_bf16, one block, a launch of 9 boards over 12 plane rows.  row_src names rows with repeats; every
    plane row that no entry below the count names is NaN, entries at or behind the count name such a NaN row.  Counts 0, 1,
    2, 3, 4, 5, 8, 9 and 12 (clamped to the launch's 9 boards), with the row map and without (board b then reads row b).
    Rows below the count equal the plain launch's rows of their source slots bit for bit; EVERY row at or behind the
    count still holds the sentinel ("boards at or beyond *n_rows are skipped") - also those that share a 2- or 4-board
    workgroup with a live row."""
    import torch
    inet, planes = trunk_setup
    G, R = TRUNK_G, TRUNK_PLANE_ROWS
    Pa, Va = _trunk(L, inet, variant, planes, R, R + 1)                   # the plain launch: every plane row, clean
    assert (Pa[R] == SENT16).all() and (Va[R] == SENT16).all() and not (Pa[:R] == SENT16).any()
    assert len({r.tobytes() for r in Pa[:R].cpu().numpy()}) == R          # the rows differ: a wrong source row shows
    for use_map in (True, False):
        for n in (0, 1, 2, 3, 4, 5, 8, 9, 12):
            eff = min(n, G)
            src = [TRUNK_ROW_SRC[b] if (b < eff and use_map) else (b if b < eff else TRUNK_NAN_ROW) for b in range(G)]
            named = set(src[:eff])
            poisoned = _i16(planes.clone()).view(R, -1)
            for r in range(R):
                if r not in named:
                    poisoned[r] = NAN16
            assert TRUNK_NAN_ROW not in named or not use_map
            row_src = torch.tensor(src, device="cuda", dtype=torch.int32) if use_map else None
            Pm, Vm = _trunk(L, inet, variant, poisoned, G, G + 3, row_src=row_src, n_rows=_count(n))
            idx = torch.tensor(src[:eff], device="cuda", dtype=torch.long)
            tag = (variant, use_map, n)
            assert torch.equal(Pm[:eff], Pa[idx]) and torch.equal(Vm[:eff], Va[idx]), tag
            assert (Pm[eff:] == SENT16).all(), "rows at or behind the count were written (policy activations) %s" % (tag,)
            assert (Vm[eff:] == SENT16).all(), "rows at or behind the count were written (value activations) %s" % (tag,)


# ------------------------------------------------------------------------------------------------ policy FC
FC_M = 520
FC_COUNTS = (0, 1, 255, 256, 257, 511, 512, 513, 520, 600)
FC_SHAPES = ((384, 128), (2304, 2880))


def _fc_operands(N, K):
    import torch
    g = torch.Generator(device="cuda").manual_seed(1000 + N + K)
    act = (torch.randn(FC_M, K, device="cuda", generator=g) * 0.7).to(torch.bfloat16)      # both signs
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g) * 0.3
    assert (act.float() < 0).float().mean().item() > 0.4
    return act, w, bias


def _fc(L, variant, act, w, bias, N, K, out_rows, n_rows=None):
    import torch
    from chinesechessai_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((out_rows, N), SENT16, device="cuda", dtype=torch.int16)
    L.xq_policy_fc_set_variant(variant)
    try:
        _lib.check(L.xq_policy_fc_bf16(st, act.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), FC_M, N, K,
                                       None if n_rows is None else n_rows.data_ptr()))
        torch.cuda.synchronize()
    finally:
        L.xq_policy_fc_set_variant(-1)
    return out


@pytest.mark.parametrize("N,K", FC_SHAPES)
@pytest.mark.parametrize("variant", (0, 1))
def test_policy_fc_count_at_tile_edges(L, variant, N, K):
    """xq_policy_fc_bf16 (both kernels), 520 rows of signed activations: counts 0, 1, one either side of the 256-row tile
    edges, the launch's own 520 and 600 (clamped).  Activation rows at or behind the count are NaN.  Rows below the count
    are bit-equal to the plain launch, rows behind it hold the sentinel."""
    import torch
    act, w, bias = _fc_operands(N, K)
    plain = _fc(L, variant, act, w, bias, N, K, FC_M + 1)
    assert (plain[FC_M] == SENT16).all() and not (plain[:FC_M] == SENT16).any()
    for n in FC_COUNTS:
        eff = min(n, FC_M)
        poisoned = _i16(act.clone())
        poisoned[eff:] = NAN16
        out = _fc(L, variant, poisoned.view(torch.bfloat16), w, bias, N, K, FC_M + 1, n_rows=_count(n))
        assert torch.equal(out[:eff], plain[:eff]), (variant, N, K, n)
        assert (out[eff:] == SENT16).all(), "rows at or behind the count were written %s" % ((variant, N, K, n),)


@pytest.mark.parametrize("N,K", FC_SHAPES)
def test_policy_fc_against_float64_per_element(L, N, K):
    """Both FC kernels against act.double() @ w.double().T + bias on the CPU, element by element:
    |out - ref| <= 2^-8 |ref| + K 2^-24 sum_k |act w| - one bf16 ulp of the result plus the a-priori bound of a K-term
    fp32 chain (the products of two bf16 are exact in fp32), every term computed from the operands in float64.  A wrong
    small logit fails this where a tolerance scaled by the matrix's largest output would pass it."""
    import torch
    act, w, bias = _fc_operands(N, K)
    a64, w64 = act.double().cpu(), w.double().cpu()
    ref = a64 @ w64.T + bias.double().cpu()
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * (a64.abs() @ w64.abs().T)
    for variant in (0, 1):
        out = _fc(L, variant, act, w, bias, N, K, FC_M)
        err = (out.view(torch.bfloat16).double().cpu() - ref).abs()
        ratio = float((err / bound).max())
        print("policy FC variant %d (N, K) = (%d, %d): largest error / bound = %.3f" % (variant, N, K, ratio))
        assert bool((err <= bound).all()), (variant, N, K, ratio)


# ------------------------------------------------------------------------------------------------ value head
VH_M = 70
VH_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 70, 99)


def _vh_operands():
    import torch
    g = torch.Generator(device="cuda").manual_seed(4242)
    hv = torch.relu(torch.randn(VH_M, 720, device="cuda", generator=g)).to(torch.bfloat16)        # behind a ReLU, as the trunk writes it
    w1 = torch.zeros(128, 736, device="cuda", dtype=torch.bfloat16)
    w1[:, :720] = (torch.randn(128, 720, device="cuda", generator=g) * 0.04).to(torch.bfloat16)
    b1 = torch.randn(128, device="cuda", generator=g) * 0.1
    w2 = torch.randn(128, device="cuda", generator=g) * 0.04
    b2 = torch.randn(1, device="cuda", generator=g) * 0.1
    return hv, w1, b1, w2, b2


def _vh(L, flat, ops, n_rows=None):
    """flat: int16 [VH_M * 720 + 16] - the activations and the 32-byte slack behind the last row, nothing more"""
    import torch
    from chinesechessai_amd import _lib
    _, w1, b1, w2, b2 = ops
    assert flat.numel() == VH_M * 720 + 16
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((VH_M + 2,), SENT16, device="cuda", dtype=torch.int16)
    _lib.check(L.xq_value_head_bf16(st, flat.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                    out.data_ptr(), VH_M, None if n_rows is None else n_rows.data_ptr()))
    torch.cuda.synchronize()
    return out


def _vh_flat(hv, eff, poison):
    """the activations with rows >= eff (and the slack) clean-zero, or poisoned: alternately the largest finite bf16 and
    stale-looking finite garbage"""
    import torch
    flat = torch.zeros(VH_M * 720 + 16, device="cuda", dtype=torch.int16)
    flat[:VH_M * 720] = _i16(hv).reshape(-1)
    if poison:
        g = torch.Generator(device="cuda").manual_seed(99)
        tail = flat[eff * 720:]
        garbage = _i16((torch.randn(tail.numel(), device="cuda", generator=g) * 37.0).to(torch.bfloat16))
        tail.copy_(torch.where(torch.arange(tail.numel(), device="cuda") % 2 == 0, torch.full_like(garbage, MAXF16), garbage))
        assert bool(torch.isfinite(tail.view(torch.bfloat16).float()).all())
    return flat


def test_value_head_count_and_finite_stale_rows(L):
    """xq_value_head_bf16, 70 rows: counts 0, 1, one either side of the 16-row wave and the 64-row workgroup edges, the
    launch's own 70 and 99 (clamped).  Rows at or behind the count - and the 32-byte slack behind row 69 - hold the largest
    finite bf16 and finite garbage (what a stale row of an earlier round looks like; not NaN: the 16 values behind a
    computed row are read and meet zero weights, include/xq_selfplay.h).  Values below the count are bit-equal to the plain
    launch on clean data, values behind it hold the sentinel."""
    import torch
    ops = _vh_operands()
    plain = _vh(L, _vh_flat(ops[0], VH_M, False), ops)
    assert (plain[VH_M:] == SENT16).all() and not (plain[:VH_M] == SENT16).any()
    assert len(set(plain[:VH_M].cpu().tolist())) > VH_M // 2
    for n in VH_COUNTS:
        eff = min(n, VH_M)
        out = _vh(L, _vh_flat(ops[0], eff, True), ops, n_rows=_count(n))
        assert torch.equal(out[:eff], plain[:eff]), n
        assert (out[eff:] == SENT16).all(), "values at or behind the count were written (count %d)" % n


def test_value_head_against_float64_per_element(L):
    """tanh(w2 . relu(w1 . hv + b1) + b2) in float64 on the CPU; per value
    |out - ref| <= 2^-8 |ref| + e2 + 4 2^-24, where e1_j = 736 2^-24 (sum_k |hv w1_jk| + |b1_j|) bounds hidden unit j's
    736-term fp32 chain, e2 = sum_j |w2_j| e1_j + 129 2^-24 (sum_j |h_j w2_j| + |b2|) carries it through the ReLU (1-Lipschitz)
    and adds the 128-term fp32 dot product and the bias add, tanh passes e2 on (derivative <= 1), 4 2^-24 is tanhf's error
    and 2^-8 |ref| the bf16 rounding of the result.  Every term comes from the operands."""
    import torch
    ops = _vh_operands()
    hv, w1, b1, w2, b2 = (t.double().cpu() for t in ops)
    pre = hv @ w1[:, :720].T + b1
    h = pre.clamp(min=0)
    s = h @ w2 + b2
    ref = torch.tanh(s)
    u = 2.0 ** -24
    e1 = 736 * u * (hv.abs() @ w1[:, :720].abs().T + b1.abs())
    e2 = e1 @ w2.abs() + 129 * u * ((h * w2).abs().sum(dim=1) + b2.abs())
    bound = 2.0 ** -8 * ref.abs() + e2 + 4 * u
    out = _vh(L, _vh_flat(ops[0], VH_M, False), ops)[:VH_M].view(torch.bfloat16).double().cpu()
    err = (out - ref).abs()
    ratio = float((err / bound).max())
    print("value head: largest error / bound = %.3f" % ratio)
    assert bool((err <= bound).all()), ratio
    assert float(ref.abs().max()) < 0.999 and float(ref.abs().max()) > 0.05          # not saturated, not all zero


def test_head_buffers_hand_out_a_zeroed_slack(L):
    """InferenceNet._head_buffers: the value activations' buffer ends in slack the value head may read - at least the 16
    bf16 values behind the last row - and that slack is zero-initialised (finite), as include/xq_selfplay.h asks."""
    import torch
    from chinesechessai_amd.neural_network import ChessNet, InferenceNet
    inet = InferenceNet(ChessNet(num_blocks=1).eval().cuda())
    for g in (5, 64):
        hp, hv = inet._head_buffers(g, torch.device("cuda"))
        flat = inet._hbuf[2]
        assert hv.shape == (g, 720) and hv.data_ptr() == flat.data_ptr() and hv.is_contiguous()
        slack = flat[g * 720:]
        assert slack.numel() >= 16 and bool((slack.view(torch.int16) == 0).all())
