"""GPU tests (`-m gpu`): every bf16 trunk kernel, the per-layer path and the policy FC on integer-valued networks
(tests/exact_trunk.py), against a float64 restatement on the CPU, bit for bit.  Integer weights, biases and 0 / 1 planes
make every fp32 partial sum exact in any order (sum of |terms| < 2^24, asserted for every case), so the one bf16 rounding
per layer is a function of an exact number and the kernel has no freedom left: no tolerance anywhere in this file."""
import functools
import math

import pytest

from tests import exact_trunk as X
from tests.test_gpu_tower256 import SENT, L, _planes  # noqa: F401  (L: the library fixture)

pytestmark = pytest.mark.gpu

# the single-launch trunk entries: name -> (channels, C entry, build selected through xq_tower_set_variant or None)
KERNELS = {"tower64": (64, "xq_tower64_nhwc_bf16", None), "tower192": (192, "xq_tower192_nhwc_bf16", None),
           "tower256": (256, "xq_tower256_nhwc_bf16", None), "tower128-36": (128, "xq_tower_nhwc_bf16", 36),
           "tower128-39": (128, "xq_tower_nhwc_bf16", 39), "tower128-60": (128, "xq_tower_nhwc_bf16", 60),
           "tower128-0": (128, "xq_tower_nhwc_bf16", 0)}
TRUNK_CASES = [(name,) + case for name, (channels, _, _) in KERNELS.items() for case in X.trunk_cases(channels)]


@pytest.fixture(scope="module", autouse=True)
def _selectors_back_at_their_defaults(L):
    yield
    L.xq_tower_set_variant(-1)
    L.xq_conv3x3_set_variant(1)
    L.xq_policy_fc_set_variant(-1)


@functools.lru_cache(maxsize=None)
def _reference(channels, blocks, k, G, per_layer=False):
    """The integer network on the device, the planes, and the chain on the CPU; one per case, shared by the builds of
    the 128-channel kernel, and left unchanged by every test."""
    t = X.integer_net(channels, blocks, k, X.NET_SEED)
    planes = _planes(G, X.PLANES_SEED)
    ch = (X.per_layer_chain if per_layer else X.float64_chain)(t, planes.cpu(), blocks)
    assert ch.headroom < X.EXACT, "C=%d blocks=%d: headroom 2^%.1f" % (channels, blocks, math.log2(ch.headroom))
    if blocks:
        assert ch.changed >= 100 and ch.ties >= 20
    return X.IntegerNet(*(x.cuda() for x in t)), planes, ch


def _tower(L, entry, t, planes, G, blocks):
    import torch
    from chinesechessai_amd import _lib
    P = torch.full((G + 1, 2880), SENT, device="cuda", dtype=torch.int16)
    V = torch.full((G + 1, 720), SENT, device="cuda", dtype=torch.int16)
    _lib.check(getattr(L, entry)(torch.cuda.current_stream().cuda_stream, planes.data_ptr(), t.w1.data_ptr(), t.wt.data_ptr(),
                                 t.bias.data_ptr(), t.wh.data_ptr(), t.bh.data_ptr(), P.data_ptr(), V.data_ptr(), G, blocks,
                                 None, None))
    torch.cuda.synchronize()
    return P, V


def _heads(P, V, G):
    """[G, 90, 40] int16: the policy head's 32 channels, then the value head's 8, of the first G rows; the sentinel row
    behind them must be whole."""
    import torch
    assert (P[G] == SENT).all() and (V[G] == SENT).all(), "the row behind the last board was written"
    return torch.cat([P[:G].view(G, 90, 32), V[:G].view(G, 90, 8)], dim=2).cpu()


@pytest.mark.parametrize("name,blocks,k,G", TRUNK_CASES)
def test_trunk_equals_float64_chain_bit_for_bit(L, name, blocks, k, G):
    """Every single-launch bf16 trunk kernel and every selectable build of the 128-channel one: no tower, one dense
    block at one board, one board into the second and into the third workgroup, 2, 6 and 20 blocks."""
    channels, entry, variant = KERNELS[name]
    t, planes, ch = _reference(channels, blocks, k, G)
    try:
        if variant is not None:
            L.xq_tower_set_variant(variant)
        P, V = _tower(L, entry, t, planes, G, blocks)
    finally:
        L.xq_tower_set_variant(-1)
    diff = X.first_difference(_heads(P, V, G), ch.bits)
    assert diff is None, "%s blocks=%d G=%d: %s" % (name, blocks, G, diff)


@pytest.mark.parametrize("blocks,k", ((1, X.DENSE), (6, 6)))
def test_trunk256_on_padded_192_channel_net_equals_trunk192(L, blocks, k):
    """k_tower256 on the 192-channel integer network, zero-padded to 256 channels, against k_tower192 on the network
    itself: the padded channels are relu(0 + 0) = 0 and meet zero weights, so both compute the chain's bits."""
    import torch
    import torch.nn.functional as F
    G = X.BOARDS[192][1]
    t, planes, ch = _reference(192, blocks, k, G)
    padded = X.IntegerNet(F.pad(t.w1, (0, 0, 0, 64)).contiguous(), F.pad(t.wt, (0, 64, 0, 64)).contiguous(),
                          F.pad(t.bias, (0, 64)).contiguous(), F.pad(t.wh, (0, 64)).contiguous(), t.bh)
    assert padded.w1.shape == (9, 256, 16) and padded.wt.shape == (2 * blocks, 9, 256, 256) and padded.wh.shape == (64, 256)
    h192 = _heads(*_tower(L, "xq_tower192_nhwc_bf16", t, planes, G, blocks), G)
    h256 = _heads(*_tower(L, "xq_tower256_nhwc_bf16", padded, planes, G, blocks), G)
    diff = X.first_difference(h256, h192)
    assert diff is None, "k_tower256 (padded) against k_tower192, blocks=%d: %s" % (blocks, diff)
    assert torch.equal(h192, ch.bits)


@pytest.mark.parametrize("variant", (1, 2))
@pytest.mark.parametrize("blocks,k,G", ((1, X.DENSE, 1), (1, X.DENSE, 5), (2, 24, 1), (2, 24, 5)))
def test_per_layer_path_equals_its_chain_bit_for_bit(L, variant, blocks, k, G):
    """xq_conv3x3_nhwc_bf16 (both builds; c_in 16, then 128) per convolution and xq_heads_nhwc_bf16, against the chain
    in the per-layer kernel's own order: conv + bias rounded, then the skip added and the sum rounded again."""
    import torch
    from chinesechessai_amd import _lib
    t, planes, ch = _reference(128, blocks, k, G, per_layer=True)
    st = torch.cuda.current_stream().cuda_stream
    a, b, c = (torch.full((G + 1, 10, 9, 128), SENT, device="cuda", dtype=torch.int16) for _ in range(3))
    P = torch.full((G + 1, 2880), SENT, device="cuda", dtype=torch.int16)
    V = torch.full((G + 1, 720), SENT, device="cuda", dtype=torch.int16)

    def conv(src, dst, w, bias, res, cin):
        _lib.check(L.xq_conv3x3_nhwc_bf16(st, src.data_ptr(), w.data_ptr(), bias.data_ptr(),
                                          None if res is None else res.data_ptr(), dst.data_ptr(), G, cin, 1))
    try:
        L.xq_conv3x3_set_variant(variant)
        conv(planes, a, t.w1, t.bias[0], None, 16)
        cur, t1, t2 = a, b, c
        for i in range(blocks):
            conv(cur, t1, t.wt[2 * i], t.bias[1 + 2 * i], None, 128)
            conv(t1, t2, t.wt[2 * i + 1], t.bias[2 + 2 * i], cur, 128)
            cur, t2 = t2, cur
        _lib.check(L.xq_heads_nhwc_bf16(st, cur.data_ptr(), t.wh.data_ptr(), t.bh.data_ptr(), P.data_ptr(), V.data_ptr(), G))
        torch.cuda.synchronize()
    finally:
        L.xq_conv3x3_set_variant(1)
    for buf in (a, b, c):
        assert (buf[G] == SENT).all(), "a convolution wrote behind the last board"
    diff = X.first_difference(_heads(P, V, G), ch.bits)
    assert diff is None, "per-layer path, build %d, blocks=%d G=%d: %s" % (variant, blocks, G, diff)
    single = X.float64_chain(X.IntegerNet(*(x.cpu() for x in t)), planes.cpu(), blocks).bits
    assert not torch.equal(single, ch.bits), "the two orders cannot be told apart on this case"


@functools.lru_cache(maxsize=None)
def _fc_reference(rows):
    import torch
    N, K = 2304, 2880
    g = torch.Generator().manual_seed(rows)
    act = torch.randint(0, 256, (rows, K), generator=g) * (torch.rand(rows, K, generator=g) < 0.5)
    w = torch.randint(-1, 2, (N, K), generator=g)
    bias = torch.randint(-8, 9, (N,), generator=g)
    # the sum of |terms| of any output: below 2^20, so every fp32 partial sum is exact in any order
    room = (act.double() @ w.double().abs().t() + bias.double().abs()).max().item()
    assert room <= K * 255 + 8 < 2 ** 20 and K * 255 + 8 < X.EXACT
    exact = act.double() @ w.double().t() + bias.double()
    ref = X.rne(exact)
    assert int((ref != exact).sum()) >= 100 and (exact < 0).any() and (exact > 0).any()
    return (act.bfloat16().cuda(), w.bfloat16().cuda(), bias.float().cuda(), ref.bfloat16().contiguous().view(torch.int16))


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("rows", (1, 37, 257))
def test_policy_fc_equals_float64_product_bit_for_bit(L, variant, rows):
    """xq_policy_fc_bf16, both kernels, 2,304 columns, K = 2,880: activations 0..255 (each exact in bf16, half of them
    zero), dense weights from {-1, 0, 1}, biases in -8..8; one row, a ragged wave and one row into a second 256-row tile."""
    import torch
    from chinesechessai_amd import _lib
    N, K = 2304, 2880
    act, w, bias, ref = _fc_reference(rows)
    out = torch.full((rows + 1, N), SENT, device="cuda", dtype=torch.int16)
    try:
        L.xq_policy_fc_set_variant(variant)
        _lib.check(L.xq_policy_fc_bf16(torch.cuda.current_stream().cuda_stream, act.data_ptr(), w.data_ptr(), bias.data_ptr(),
                                       out.data_ptr(), rows, N, K, None))
        torch.cuda.synchronize()
    finally:
        L.xq_policy_fc_set_variant(-1)
    assert (out[rows] == SENT).all(), "the row behind the last was written"
    got = out[:rows].cpu()
    if not torch.equal(got, ref):
        d = (got != ref).nonzero()
        r, c = d[0].tolist()
        pytest.fail("policy FC kernel %d, %d rows: %d of %d outputs differ; first at row %d column %d: kernel 0x%04x, "
                    "reference 0x%04x" % (variant, rows, len(d), ref.numel(), r, c, got[r, c].item() & 0xFFFF,
                                          ref[r, c].item() & 0xFFFF))
