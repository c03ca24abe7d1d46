"""GPU test (`-m gpu`, through the C ABI) of the trunk kernel without the fourth all-padding pair, (pixel tile 5, tap 0):
k_tower1wa (variant 60) issues no tap-0 MFMA for the tile of the file-0 pixels (tools/gen_tower1wa.py: SKIP == DEAD), so
that tile's accumulators take the bias row with the selector MFMA or, behind the input convolution and a block's second
convolution, with (tap 1, K-step 0).  A left-out MFMA adds exact zeros: the outputs must stay the bits of k_tower16b<4>
(variant 39), which issues every product in the same order.  (neural_network.py:47-71,181-187.)"""
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_round5 import _trunk  # noqa: E402

G = 13          # three full workgroups of 4 boards and a ragged one


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


@pytest.fixture(scope="module")
def planes():
    """board 0: all zero - the outputs are the pure bias chain, the bias row entering tile 5 at tap 1; boards 1..10: all 15
    planes set at the file-0 pixel of rank 0..9 and nothing else - the one non-zero row sits in tile 5; boards 11, 12: dense
    random"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(21)
    x = torch.zeros(G, 90, 16, device="cuda", dtype=torch.bfloat16)
    y = torch.arange(10, device="cuda")
    x[1 + y, 9 * y, :15] = 1.0
    x[11:, :, :15] = (torch.rand(2, 90, 15, device="cuda", generator=g) < 0.3).to(torch.bfloat16)
    return x.reshape(G, 10, 9, 16).contiguous()


@pytest.mark.parametrize("blocks", [2, 6])
def test_tile5_without_tap0_keeps_the_other_builds_bits(L, planes, blocks):
    """two blocks run the loop-back section (second convolution -> next block's first) exactly once, six is the benchmark's
    depth.  BatchNorm statistics are randomised so that every bias is non-zero.  Then the engine's form of the launch: a
    permutation of the slots with a ragged count (7 rows)."""
    import torch
    from chinesechessai_amd.neural_network import ChessNet, InferenceNet
    torch.manual_seed(400 + blocks)
    net = ChessNet(num_blocks=blocks).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    inet = InferenceNet(net.cuda())
    Pa, Va = _trunk(L, inet, 60, planes, G, blocks)
    Pb, Vb = _trunk(L, inet, 39, planes, G, blocks)
    # the all-zero board: the bias chain alone gives outputs
    assert Pa[0].float().abs().max().item() > 0
    # the structured boards differ from each other: the comparison is not one of 11 equal rows
    assert len({tuple(r.tolist()) for r in Pa[:11].view(torch.int16).cpu()}) == 11
    assert torch.equal(Pa.view(torch.int16), Pb.view(torch.int16))               # (row G = the guard row, 9.0 in both)
    assert torch.equal(Va.view(torch.int16), Vb.view(torch.int16))
    assert (Pa[G] == 9.0).all() and (Va[G] == 9.0).all()

    n = 7
    g = torch.Generator(device="cuda").manual_seed(22)
    perm = torch.randperm(G, device="cuda", generator=g).to(torch.int32)
    n_rows = torch.tensor([n], device="cuda", dtype=torch.int32)
    idx = perm[:n].long()
    for variant in (60, 39):
        Pm, Vm = _trunk(L, inet, variant, planes, G, blocks, row_src=perm, n_rows=n_rows)
        assert torch.equal(Pm[:n].view(torch.int16), Pa[idx].view(torch.int16)), variant
        assert torch.equal(Vm[:n].view(torch.int16), Va[idx].view(torch.int16)), variant
        # boards at or beyond the count are skipped (include/xq_selfplay.h): also those that share a workgroup with row n - 1
        assert (Pm[n:] == 9.0).all() and (Vm[n:] == 9.0).all(), variant
