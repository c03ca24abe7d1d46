"""GPU tests (`-m gpu`) of the 192-channel single-launch trunk (csrc/xq_tower192.hip, xq_tower192_nhwc_bf16): against a
float64 chain of the same folded bf16 weights, its row arguments, and a 192-channel network through SelfPlayEngine."""
import numpy as np
import pytest

from tests.test_gpu_tower256 import SENT, L, _planes  # noqa: F401  (L: the library fixture)

pytestmark = pytest.mark.gpu
NB = 3                             # boards per workgroup


def _net192(blocks, seed):
    import torch
    from chinesechessai_amd.neural_network import ChessNet
    torch.manual_seed(seed)
    net = ChessNet(num_channels=192, num_blocks=blocks).eval()
    for m in net.modules():                                      # non-trivial running statistics
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return net.cuda()


def _launch(L, inet, planes, n_boards, out_rows, row_src=None, n_rows=None):
    import torch
    from chinesechessai_amd import _lib
    P = torch.full((out_rows, 2880), SENT, device="cuda", dtype=torch.int16)
    V = torch.full((out_rows, 720), SENT, device="cuda", dtype=torch.int16)
    _lib.check(L.xq_tower192_nhwc_bf16(torch.cuda.current_stream().cuda_stream, planes.data_ptr(), inet.hip_w[0].data_ptr(),
                                       inet.hip_wt.data_ptr(), inet.hip_bt.data_ptr(), inet.hip_hw.data_ptr(),
                                       inet.hip_hb.data_ptr(), P.data_ptr(), V.data_ptr(), n_boards, inet.n_blocks,
                                       None if row_src is None else row_src.data_ptr(),
                                       None if n_rows is None else n_rows.data_ptr()))
    torch.cuda.synchronize()
    return P, V


# (1, 1) first: a cold device.  No tower at all, a workgroup with an empty slot, exactly one workgroup, one board into the
# next workgroup, several workgroups with a ragged tail, depth
@pytest.mark.parametrize("blocks,G", ((1, 1), (0, NB + 2), (1, NB - 1), (1, NB), (1, NB + 1), (2, 3 * NB + 1), (6, 37), (20, 3)))
def test_trunk192_against_float64_chain(L, blocks, G):
    """The kernel against F.conv2d in float64 on the same folded bf16 weights, activations rounded to bf16 between layers,
    the skip added before the rounding.  Bound: one bf16 ulp per rounding point on the path."""
    import torch
    import torch.nn.functional as F
    from chinesechessai_amd.neural_network import InferenceNet
    inet = InferenceNet(_net192(blocks, 10 + blocks))
    assert inet.use_hip_conv and inet.supports_row_map and inet.folded_weights()[1].shape == (2 * blocks, 9, 192, 192)
    planes = _planes(G, 5)
    P, V = _launch(L, inet, planes, G, G + 1)
    assert (P[G] == SENT).all() and (V[G] == SENT).all() and P[:G].abs().max().item() > 0 and V[:G].abs().max().item() > 0

    def conv(x, i):
        w = inet.hip_w[i].double().reshape(3, 3, 192, -1).permute(2, 3, 0, 1)
        return F.conv2d(x, w, inet.hip_b[i].double(), padding=1)

    def rnd(x):
        return torch.relu(x).bfloat16().double()
    a = rnd(conv(planes.permute(0, 3, 1, 2).double(), 0))
    for i in range(blocks):
        y = rnd(conv(a, 1 + 2 * i))
        a = rnd(conv(y, 2 + 2 * i) + a)
    ref = torch.relu(a.permute(0, 2, 3, 1).reshape(G, 90, 192) @ inet.hip_hw.double().t() + inet.hip_hb.double())
    bound = 2 ** -8 * max(1.0, ref.abs().max().item()) * (2 + blocks)
    ep = (P[:G].view(torch.bfloat16).double().view(G, 90, 32) - ref[..., :32]).abs().max().item()
    ev = (V[:G].view(torch.bfloat16).double().view(G, 90, 8) - ref[..., 32:40]).abs().max().item()
    print("trunk192 blocks=%d G=%d: largest error / bound = %.4f (policy) %.4f (value)" % (blocks, G, ep / bound, ev / bound))
    assert ep <= bound and ev <= bound


@pytest.fixture(scope="module")
def rows_setup(L):
    from chinesechessai_amd.neural_network import InferenceNet
    inet = InferenceNet(_net192(1, 77))
    planes = _planes(2 * NB + 2, 8)
    return inet, planes, _launch(L, inet, planes, 2 * NB + 2, 2 * NB + 3)


@pytest.mark.parametrize("n", (0, 1, NB - 1, NB, NB + 1, 2 * NB + 1, 2 * NB + 5))
def test_trunk192_row_map_and_count(L, rows_setup, n):
    """8 boards; row_src permutes the plane rows with one source repeated; rows no entry below the count names are NaN."""
    import torch
    inet, planes, (Pa, Va) = rows_setup
    G, src = 2 * NB + 2, (4, 0, 7, 7, 2, 6, 1, 5)
    assert (Pa[G] == SENT).all() and len({r.tobytes() for r in Pa[:G].cpu().numpy()}) == G
    eff = min(n, G)
    poisoned = planes.clone()
    for r in set(range(G)) - set(src[:eff]):
        poisoned[r] = float("nan")
    Pm, Vm = _launch(L, inet, poisoned, G, G + 3, row_src=torch.tensor(src, device="cuda", dtype=torch.int32),
                     n_rows=torch.tensor([n], device="cuda", dtype=torch.int32))
    idx = torch.tensor(src[:eff], device="cuda", dtype=torch.long)
    assert torch.equal(Pm[:eff], Pa[idx]) and torch.equal(Vm[:eff], Va[idx])
    if eff > 3:
        assert torch.equal(Pm[2], Pm[3]) and torch.equal(Vm[2], Vm[3])
    assert (Pm[eff:] == SENT).all() and (Vm[eff:] == SENT).all()


def test_net192_through_self_play_engine(L):
    """A 192-channel network in SelfPlayEngine without the library fallback: 64 games, 16 simulations, 3 plies, with row
    compaction, leaf dedupe and root carry-over, equal to the same games without them."""
    from chinesechessai_amd.engine import SelfPlayEngine, TorchNetEvaluator
    from chinesechessai_amd.neural_network import InferenceNet
    net = _net192(2, 0)
    assert InferenceNet(net).supports_row_map
    for kw in ({"fused_tower": False}, {"trunk": "mxfp8"}):
        with pytest.raises(ValueError):
            InferenceNet(net, **kw)
    S, seeds = 16, np.arange(64, dtype=np.uint32)
    ev = TorchNetEvaluator(net)
    eng = SelfPlayEngine(64, sims=S, planes_format=ev.planes_format, max_moves=3)
    b = eng.play(ev, seeds)
    assert eng.row_compaction and eng.leaf_dedupe and eng._carry_on
    eng.close()
    assert (b.error == 0).all() and (b.n_plies == 3).all()
    evp = TorchNetEvaluator(net, chunk=64, leaf_dedupe=False, eval_cache=False)      # chunked: one row per slot, no row map
    engp = SelfPlayEngine(64, sims=S, planes_format=evp.planes_format, max_moves=3)
    p = engp.play(evp, seeds)
    assert not (engp.row_compaction or engp.leaf_dedupe or engp._carry_on or engp.eval_cache)
    engp.close()
    for k in ("chosen", "s_counts", "s_moves", "s_z", "winner", "n_plies"):
        assert np.array_equal(getattr(b, k), getattr(p, k)), k
