"""GPU test (`-m gpu`, through the C ABI) of the trunk kernel's permuted MFMA columns and left-out all-padding taps:
k_tower1wa (variant 60) carries the file-0 pixels and the rank-0 / file-8 pixels in pixel tiles of their own and does not
issue the MFMAs of the (pixel tile, tap) pairs that read only the zero padding of the 3x3 convolution
(tools/gen_tower1wa.py: PIX_OF, SKIP).  A left-out MFMA adds exact zeros, so the outputs must stay the bits of
k_tower16b<4> (variant 39), which issues every product in the same order.  (neural_network.py:47-71,181-187.)"""
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_round5 import _trunk  # noqa: E402

G = 94          # 23 full workgroups of 4 boards and a ragged one


@pytest.fixture(scope="module")
def L():
    from chinesechessai_amd import _lib
    lib = _lib.lib()
    assert lib.xq_device_count() > 0, "no GPU visible"
    assert lib.xq_device_ok(0) == 1, "not a gfx950 device"
    return lib


@pytest.fixture(scope="module")
def planes():
    """boards 0..89: all 15 planes set at pixel i and nothing else - the one non-zero input row meets every tap of every
    neighbour alone, so every border case of every tap decides output bits by itself; boards 90..93: dense random"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.zeros(G, 90, 16, device="cuda", dtype=torch.bfloat16)
    i = torch.arange(90, device="cuda")
    x[i, i, :15] = 1.0
    x[90:, :, :15] = (torch.rand(4, 90, 15, device="cuda", generator=g) < 0.3).to(torch.bfloat16)
    return x.reshape(G, 10, 9, 16).contiguous()


@pytest.mark.parametrize("blocks", [1, 3])
def test_left_out_padding_taps_keep_the_other_builds_bits(L, planes, blocks):
    """one block runs the first tap under the input convolution's epilogue, both layers of a block and the last epilogue;
    three blocks also run the block loop.  BatchNorm statistics are randomised so that every bias is non-zero.  Then the
    engine's form of the launch: a permutation of the slots with a ragged count (61 rows)."""
    import torch
    from chinesechessai_amd.neural_network import ChessNet, InferenceNet
    torch.manual_seed(300 + blocks)
    net = ChessNet(num_blocks=blocks).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    inet = InferenceNet(net.cuda())
    Pa, Va = _trunk(L, inet, 60, planes, G, blocks)
    Pb, Vb = _trunk(L, inet, 39, planes, G, blocks)
    assert Pa[:G].float().abs().max().item() > 0
    # the single-pixel boards differ from each other: the comparison is not one of 90 equal rows
    assert len({tuple(r.tolist()) for r in Pa[:90].view(torch.int16).cpu()}) == 90
    assert torch.equal(Pa.view(torch.int16), Pb.view(torch.int16))               # (row G = the guard row, 9.0 in both)
    assert torch.equal(Va.view(torch.int16), Vb.view(torch.int16))
    assert (Pa[G] == 9.0).all() and (Va[G] == 9.0).all()

    n = 61
    g = torch.Generator(device="cuda").manual_seed(12)
    perm = torch.randperm(G, device="cuda", generator=g).to(torch.int32)
    n_rows = torch.tensor([n], device="cuda", dtype=torch.int32)
    idx = perm[:n].long()
    for variant in (60, 39):
        Pm, Vm = _trunk(L, inet, variant, planes, G, blocks, row_src=perm, n_rows=n_rows)
        assert torch.equal(Pm[:n].view(torch.int16), Pa[idx].view(torch.int16)), variant
        assert torch.equal(Vm[:n].view(torch.int16), Va[idx].view(torch.int16)), variant
        # boards at or beyond the count are skipped (include/xq_selfplay.h): also those that share a workgroup with row n - 1
        assert (Pm[n:] == 9.0).all() and (Vm[n:] == 9.0).all(), variant
