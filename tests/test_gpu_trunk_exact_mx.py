"""GPU tests (`-m gpu`): both MXFP8 trunk kernels (k_tower_mx, k_tower256_mx) on integer-valued networks
(tests/exact_trunk.py: integer_net_mx, mx_chain), against a float64 restatement on the CPU, bit for bit.  Integers stay
integers through the e4m3 quantiser under a power-of-two block scale, weights of the form +-2^j survive mx_quantize
exactly, so every product is an integer and every fp32 partial sum is exact in any order: the bf16 rounding and the
quantisation of every layer are functions of an exact number and the kernel has no freedom left.  The sum of |terms| is
asserted below X.MX_EXACT = 2^23 for every case: above it the scaled MFMA was seen to lose a product 2^15.6 times smaller
than its neighbour ("Bit-exact integer networks").  No tolerance anywhere in this file."""
import functools

import pytest

from tests import exact_trunk as X
from tests.test_gpu_tower256 import SENT, L, _planes  # noqa: F401  (L: the library fixture)
from tests.test_gpu_tower256_mx import _launch as _launch256
from tests.test_gpu_tower_mx import _launch as _launch128

pytestmark = pytest.mark.gpu

# channels -> (launch of the MXFP8 entry, the bf16 entry of the same width)
KERNELS = {128: (_launch128, "xq_tower_nhwc_bf16"), 256: (_launch256, "xq_tower256_nhwc_bf16")}
CASES = [(c,) + case for c in KERNELS for case in X.mx_cases(c)]


@functools.lru_cache(maxsize=None)
def _reference(channels, blocks, k, jmax, G):
    """The network on the device, the planes, and the chain on the CPU; one per case, left unchanged by every test.
    The headroom and the quantiser's events are asserted here, before anything is compared; in X.MX_BOUNDARY_CASES also
    that on these planes a "+1" firing at mantissa exactly 1.75 changes a head bit, so that a kernel which equals the
    chain is known not to have that rule (> 0x60 against >= 0x60 in the epilogue)."""
    t = X.integer_net_mx(channels, blocks, k, jmax, X.mx_net_seed(channels, blocks, k, jmax))
    planes = _planes(G, X.PLANES_SEED)
    ch = X.mx_chain(t, planes.cpu(), blocks)
    X.mx_assert_reached(ch, channels, blocks, k, jmax, G)
    if (blocks, k, jmax) in X.MX_BOUNDARY_CASES:
        wrong = X.mx_chain(t, planes.cpu(), blocks, mutant=X.MX_PLUS_ONE_AT_BOUNDARY)
        assert X.first_difference(wrong.bits, ch.bits) is not None, "the +1 at 1.75 does not show on these planes"
    return X.MxNet(*(x.cuda() for x in t)), planes, ch


def _heads(P, V, rows, total):
    """[rows, 90, 40] int16: the policy head's 32 channels, then the value head's 8; every row from `rows` on, the one
    behind the last board included, must be whole."""
    import torch
    assert P.shape[0] == V.shape[0] == total > rows
    assert (P[rows:] == SENT).all() and (V[rows:] == SENT).all(), "a row behind the last was written"
    return torch.cat([P[:rows].view(rows, 90, 32), V[:rows].view(rows, 90, 8)], dim=2).cpu()


@pytest.mark.parametrize("channels,blocks,k,jmax,G", CASES)
def test_mx_trunk_equals_chain_bit_for_bit(L, channels, blocks, k, jmax, G):
    """No tower, one dense block (weights x 2^0..3) at one board, one board into the second and into the third workgroup,
    (2, 24, 3), (6, 6, 0), (6, 5, 1) and (20, 2, 0) at the middle count: the "+1" rule on and at its boundary, e4m3 ties,
    subnormals, many activation and weight scale bytes, all behind sums of up to 2,304 terms."""
    t, planes, ch = _reference(channels, blocks, k, jmax, G)
    P, V = KERNELS[channels][0](L, t, planes, G, G + 1, blocks)
    diff = X.first_difference(_heads(P, V, G, G + 1), ch.bits)
    assert diff is None, "C=%d blocks=%d k=%d jmax=%d G=%d: %s" % (channels, blocks, k, jmax, G, diff)


@pytest.mark.parametrize("channels,src,n", ((128, (4, 0, 7, 7, 2, 8, 1, 5, 3), 7), (256, (3, 0, 4, 4, 1), 4)))
def test_mx_trunk_row_map_equals_chain_rows(L, channels, src, n):
    """The dense block at the largest board count: row_src permutes the plane rows with one source repeated, n_rows is
    below the board count.  Output row r must hold the chain's row src[r] in every bit, rows from n_rows on stay whole."""
    import torch
    G = X.BOARDS[channels][2]
    assert len(src) == G and len(set(src)) == G - 1 and n < G
    t, planes, ch = _reference(channels, 1, X.DENSE, 3, G)
    P, V = KERNELS[channels][0](L, t, planes, G, G + 1, 1, row_src=torch.tensor(src, device="cuda", dtype=torch.int32),
                                n_rows=torch.tensor([n], device="cuda", dtype=torch.int32))
    diff = X.first_difference(_heads(P, V, n, G + 1), ch.bits[list(src[:n])])
    assert diff is None, "C=%d row map: %s" % (channels, diff)


@pytest.mark.parametrize("channels", (128, 256))
def test_mx_trunk_without_tower_equals_bf16_trunk(L, channels):
    """With no tower nothing is quantised: the MXFP8 entry must equal the bf16 entry on the same w1 and heads in every
    bit, and both float64_chain."""
    import torch
    from chinesechessai_amd import _lib
    G = X.BOARDS[channels][1]
    t, planes, ch = _reference(channels, 0, 0, 0, G)
    launch, bf16_entry = KERNELS[channels]
    mx = _heads(*launch(L, t, planes, G, G + 1, 0), G, G + 1)
    wt = torch.zeros(0, 9, channels, channels, device="cuda", dtype=torch.bfloat16)
    P = torch.full((G + 1, 2880), SENT, device="cuda", dtype=torch.int16)
    V = torch.full((G + 1, 720), SENT, device="cuda", dtype=torch.int16)
    _lib.check(getattr(L, bf16_entry)(torch.cuda.current_stream().cuda_stream, planes.data_ptr(), t.w1.data_ptr(), wt.data_ptr(),
                                      t.bias.data_ptr(), t.wh.data_ptr(), t.bh.data_ptr(), P.data_ptr(), V.data_ptr(), G, 0,
                                      None, None))
    torch.cuda.synchronize()
    bf = _heads(P, V, G, G + 1)
    diff = X.first_difference(mx, bf)
    assert diff is None, "C=%d, no tower, MXFP8 entry against bf16 entry: %s" % (channels, diff)
    base = X.float64_chain(X.integer_net(channels, 0, 0, X.NET_SEED), planes.cpu(), 0)
    assert torch.equal(bf, base.bits) and torch.equal(mx, ch.bits)
