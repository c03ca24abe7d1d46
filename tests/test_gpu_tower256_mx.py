"""GPU tests (`-m gpu`) of the 256-channel MXFP8 single-launch trunk (csrc/xq_tower256_mx.hip, xq_tower256_mxfp8_nhwc): bit
for bit on towers whose every output is one product, against a float64 chain of the bytes it reads, its row arguments, and
through SelfPlayEngine."""
import numpy as np
import pytest

from tests.test_gpu_tower256 import SENT, L, _net256, _planes  # noqa: F401  (L: the library fixture)

pytestmark = pytest.mark.gpu
C = 256


def _launch(L, t, planes, n_boards, out_rows, blocks, row_src=None, n_rows=None):
    """t = (w1, wq, wscale, bias, wh, bh), device tensors."""
    import torch
    from chinesechessai_amd import _lib
    P = torch.full((out_rows, 2880), SENT, device="cuda", dtype=torch.int16)
    V = torch.full((out_rows, 720), SENT, device="cuda", dtype=torch.int16)
    _lib.check(L.xq_tower256_mxfp8_nhwc(torch.cuda.current_stream().cuda_stream, planes.data_ptr(), *(x.data_ptr() for x in t),
                                        P.data_ptr(), V.data_ptr(), n_boards, blocks,
                                        None if row_src is None else row_src.data_ptr(),
                                        None if n_rows is None else n_rows.data_ptr()))
    torch.cuda.synchronize()
    return P, V


def _tensors(inet):
    return (inet.hip_w[0], inet.hip_wq, inet.hip_ws, inet.hip_bt, inet.hip_hw, inet.hip_hb)


def _chain(t, planes, blocks, dt, ch=C):
    """The trunk of width `ch` restated in torch on the CPU, accumulating in `dt`: convolutions on mx_dequantize of the weight
    bytes and of mx_quantize applied to the bf16-rounded activations, the skip added before the rounding.  Returns the head
    activations [G, 90, 64] before their bf16 rounding."""
    import torch
    import torch.nn.functional as F
    from chinesechessai_amd.neural_network import mx_dequantize, mx_quantize
    w1, wq, ws, bias, wh, bh = (x.cpu() for x in t)

    def rnd(x):
        return torch.relu(x).bfloat16().to(dt)

    def convq(x, i, start):                                          # start: bias (+ skip), the accumulator's first value
        xq = mx_dequantize(*mx_quantize(x.permute(0, 2, 3, 1).contiguous())).permute(0, 3, 1, 2)
        w = mx_dequantize(wq[i], ws[i]).reshape(3, 3, ch, ch).permute(2, 3, 0, 1)
        return start + F.conv2d(xq, w, None, padding=1).to(dt)       # (the convolution itself in float64)
    a = rnd(F.conv2d(planes.cpu().permute(0, 3, 1, 2).to(dt), w1.to(dt).reshape(3, 3, ch, 16).permute(2, 3, 0, 1),
                     bias[0].to(dt), padding=1))
    for i in range(blocks):
        y = rnd(convq(a, 2 * i, bias[1 + 2 * i].to(dt).view(1, -1, 1, 1)))
        a = rnd(convq(y, 2 * i + 1, bias[2 + 2 * i].to(dt).view(1, -1, 1, 1) + a))
    return torch.relu(a.permute(0, 2, 3, 1).reshape(-1, 90, ch) @ wh.to(dt).t() + bh.to(dt))


@pytest.mark.parametrize("blocks,G", ((1, 1), (2, 3), (1, 5)))
def test_trunk256_mx_one_hot_towers_bit_for_bit(L, blocks, G):
    """test_trunk_mx_one_hot_towers_bit_for_bit's construction at 256 channels: every tower output channel has one non-zero
    weight (one tap, one input channel, +-2^k, k in -2..2), bias 0; w1 and its bias are multiples of 2^-6; every head channel
    has one random bf16 weight.  Every output is one product plus at most one addend, whatever the order: a float32
    restatement must equal P and V in every bit.  A cin in another 32-block or the other K-half than the kernel's operand
    and scale layout assumes comes out wrong here.  G = 1 and odd G leave the workgroup's second board slot empty."""
    import torch
    from chinesechessai_amd.neural_network import mx_quantize
    g = torch.Generator().manual_seed(100 * blocks + G)
    n = 2 * blocks

    def one_hot(shape_rows, n_cols, values):                         # [..., row, col]: one value per row
        w = torch.zeros(shape_rows + (n_cols,), dtype=torch.float64)
        w.view(-1, n_cols).scatter_(1, torch.randint(0, n_cols, (values.numel(), 1), generator=g), values.reshape(-1, 1))
        return w
    w1 = torch.randint(-16, 17, (9, C, 16), generator=g).double() / 64
    val = torch.ldexp(torch.ones(n, C, dtype=torch.float64), torch.randint(-2, 3, (n, C), generator=g)) * (
        torch.randint(0, 2, (n, C), generator=g) * 2 - 1)
    wt = one_hot((n, C), 9 * C, val).view(n, C, 9, C).permute(0, 2, 1, 3).contiguous()      # [layer][tap][cout][cin]
    bias = torch.zeros(1 + n, C)
    bias[0] = torch.randint(-32, 33, (C,), generator=g).float() / 64
    wh = torch.zeros(64, C, dtype=torch.float64)
    wh[:40] = one_hot((40,), C, torch.randn(40, generator=g).bfloat16().double())
    bh = torch.zeros(64)
    bh[:40] = torch.randn(40, generator=g)
    wq, ws = mx_quantize(wt)
    t = tuple(x.cuda().contiguous() for x in (w1.bfloat16(), wq, ws, bias, wh.bfloat16(), bh))
    planes = _planes(G, 40 + G)
    P, V = _launch(L, t, planes, G, G + 1, blocks)
    ref = _chain(t, planes, blocks, torch.float32).bfloat16().view(torch.int16)
    assert ref[..., :40].abs().max().item() > 0 and (P[G] == SENT).all() and (V[G] == SENT).all()
    assert torch.equal(P[:G].cpu().view(G, 90, 32), ref[..., :32]) and torch.equal(V[:G].cpu().view(G, 90, 8), ref[..., 32:40])


@pytest.mark.parametrize("blocks,G", ((1, 1), (0, 5), (1, 2), (2, 3), (6, 37), (20, 3)))     # (1, 1) first: a cold device
def test_trunk256_mx_against_float64_chain(L, blocks, G):
    """The kernel against F.conv2d in float64 on mx_dequantize of the very bytes it reads, the quantiser applied to the
    bf16-rounded activations.  Bound: test_trunk256_against_float64_chain's and test_trunk_mx_against_float64_chain's, one
    bf16 ulp per rounding point on the path.  Largest error / bound on an MI355X (the larger of policy and value): 0.16, 0.24,
    0.16, 0.14, 0.43, 0.56."""
    import torch
    from chinesechessai_amd.neural_network import InferenceNet
    inet = InferenceNet(_net256(blocks, 10 + blocks), trunk="mxfp8_256")
    assert inet.supports_row_map and [x.shape for x in inet.folded_weights()[-2:]] == [(2 * blocks, 9, C, C), (2 * blocks, 9, C, 8)]
    assert inet.folded_weights()[1].shape[0] == 0                     # the bf16 tower weights are not uploaded
    planes = _planes(G, 5)
    P, V = _launch(L, _tensors(inet), planes, G, G + 1, blocks)
    assert (P[G] == SENT).all() and (V[G] == SENT).all() and P[:G].abs().max().item() > 0 and V[:G].abs().max().item() > 0
    ref = _chain(_tensors(inet), planes, blocks, torch.float64)
    bound = 2 ** -8 * max(1.0, ref.abs().max().item()) * (2 + blocks)
    ep = (P[:G].cpu().view(torch.bfloat16).double().view(G, 90, 32) - ref[..., :32]).abs().max().item()
    ev = (V[:G].cpu().view(torch.bfloat16).double().view(G, 90, 8) - ref[..., 32:40]).abs().max().item()
    print("trunk mxfp8_256 blocks=%d G=%d: largest error / bound = %.4f (policy) %.4f (value)" % (blocks, G, ep / bound, ev / bound))
    assert ep <= bound and ev <= bound


@pytest.fixture(scope="module")
def rows_setup(L):
    from chinesechessai_amd.neural_network import InferenceNet
    inet = InferenceNet(_net256(1, 77), trunk="mxfp8_256")
    planes = _planes(9, 8)
    return inet, planes, _launch(L, _tensors(inet), planes, 9, 10, 1)


@pytest.mark.parametrize("n", (0, 1, 2, 3, 8, 9, 12))
def test_trunk256_mx_row_map_and_count(L, rows_setup, n):
    """9 boards; row_src permutes the plane rows with one source repeated; rows no entry below the count names are NaN."""
    import torch
    inet, planes, (Pa, Va) = rows_setup
    G, src = 9, (4, 0, 7, 7, 2, 8, 1, 5, 3)
    assert (Pa[G] == SENT).all() and len({r.tobytes() for r in Pa[:G].cpu().numpy()}) == G
    eff = min(n, G)
    poisoned = planes.clone()
    for r in set(range(G)) - set(src[:eff]):
        poisoned[r] = float("nan")
    Pm, Vm = _launch(L, _tensors(inet), poisoned, G, G + 3, 1, row_src=torch.tensor(src, device="cuda", dtype=torch.int32),
                     n_rows=torch.tensor([n], device="cuda", dtype=torch.int32))
    idx = torch.tensor(src[:eff], device="cuda", dtype=torch.long)
    assert torch.equal(Pm[:eff], Pa[idx]) and torch.equal(Vm[:eff], Va[idx])
    if eff > 3:
        assert torch.equal(Pm[2], Pm[3]) and torch.equal(Vm[2], Vm[3])
    assert (Pm[eff:] == SENT).all() and (Vm[eff:] == SENT).all()


def test_mx256_trunk_through_self_play_engine(L):
    """TorchNetEvaluator(net, trunk="mxfp8_256") in SelfPlayEngine: 64 games, 16 simulations, 3 plies, with row compaction,
    leaf dedupe and root carry-over, equal to the same games chunked without them; configurations the kernel does not cover
    raise."""
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import ChessNet, InferenceNet
    net = _net256(2, 0)
    for bad in (lambda: InferenceNet(ChessNet(num_channels=128, num_blocks=1).eval().cuda(), trunk="mxfp8_256"),
                lambda: InferenceNet(net, trunk="mxfp8_256", fused_tower=False),
                lambda: TorchNetEvaluator(InferenceNet(net), trunk="mxfp8_256"),
                lambda: TorchNetEvaluator(InferenceNet(net, trunk="mxfp8_256"))):
        with pytest.raises(ValueError):
            bad()
    S, seeds = 16, np.arange(64, dtype=np.uint32)
    ev = TorchNetEvaluator(net, trunk="mxfp8_256")
    assert ev.inet.trunk == "mxfp8_256"
    eng = SelfPlayEngine(64, sims=S, planes_format=ev.planes_format, max_moves=3)
    b = eng.play(ev, seeds)
    assert eng.row_compaction and eng.leaf_dedupe and eng._carry_on
    eng.close()
    assert (b.error == 0).all() and (b.n_plies == 3).all()
    evp = TorchNetEvaluator(net, chunk=64, leaf_dedupe=False, eval_cache=False, trunk="mxfp8_256")   # one row per slot, no row map
    engp = SelfPlayEngine(64, sims=S, planes_format=evp.planes_format, max_moves=3)
    p = engp.play(evp, seeds)
    assert not (engp.row_compaction or engp.leaf_dedupe or engp._carry_on or engp.eval_cache)
    engp.close()
    for k in ("chosen", "s_counts", "s_moves", "s_z", "winner", "n_plies"):
        assert np.array_equal(getattr(b, k), getattr(p, k)), k
