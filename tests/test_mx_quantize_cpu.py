"""mx_quantize / mx_dequantize (neural_network.py) on the CPU: the MXFP8 rule of csrc/xq_tower_mx.hip on hand-made blocks."""
import math

import pytest
import torch

from chinesechessai_amd.neural_network import mx_dequantize, mx_quantize


def _block(**at):
    x = torch.zeros(32, dtype=torch.float64)
    for i, v in at.items():
        x[int(i[1:])] = v
    return x


g = torch.Generator().manual_seed(3)
CASES = {
    "all_zero": (_block(), True),
    "single_one": (_block(i5=1.0), True),
    "max_448_pow2": (_block(i0=448.0 * 2 ** 5, i1=-15 * 2.0 ** 6), True),          # 448 * 2^k exactly: no "+1"
    "max_above_448_pow2": (_block(i0=449.0 * 2 ** 5, i1=7 * 2.0 ** 8), False),       # the "+1" rule fires
    # 2^-9 of the maximum and below it, down to the subnormals: 2^-9 is the last bit, 2^-10 and -1.5 * 2^-9 are ties
    "tiny_beside_max": (_block(i0=256.0, i1=2.0 ** -1, i2=2.0 ** -2, i3=2.0 ** -9, i4=2.0 ** -10, i5=-3 * 2.0 ** -10), False),
    "mixed_signs": (_block(i0=-3.0, i1=2.5, i2=-0.625, i31=1.75), True),
    "axis_128": (torch.randn(3, 128, generator=g, dtype=torch.float64) * torch.tensor([1e-3, 1.0, 300.0]).view(3, 1), False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_mx_quantize_blocks(name):
    x, exact = CASES[name]
    q, s = mx_quantize(x)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8 and q.shape == x.shape and s.shape == x.shape[:-1] + (x.shape[-1] // 32,)
    assert not ((q & 0x7F) == 0x7F).any()                                 # no NaN byte (0x7F, 0xFF)
    xd = x.double().reshape(-1, 32)
    for blk, byte in zip(xd, s.reshape(-1).tolist()):                     # the rule in Python integers / exact floats
        m = float(blk.abs().max())
        if m == 0:
            want = 127
        else:
            e = math.frexp(m)[1] - 1 - 8
            if m * 2.0 ** -e > 448:
                e += 1
            want = min(max(e + 127, 0), 254)
            assert 224 < m * 2.0 ** -(want - 127) <= 448
        assert byte == want
    back = mx_dequantize(q, s)
    assert back.dtype == torch.float64 and back.shape == x.shape
    if exact:                                                             # values k * 2^e, |k| <= 15, within the block's range
        assert torch.equal(back, x.double())
    # elsewhere within half an e4m3 step at the block's scale: the step of the binade of |y| = |x| * 2^-e, 2^-9 below 2^-6
    e = (s.to(torch.int64) - 127).reshape(-1, 1)
    y = torch.ldexp(xd, -e).abs()
    step = torch.ldexp(torch.ones_like(y), (torch.frexp(y)[1] - 1).clamp(min=-6).to(torch.int64) - 3 + e)
    assert ((back.reshape(-1, 32) - xd).abs() <= step / 2).all()
    if name == "tiny_beside_max":
        assert s.tolist() == [127] and q[:6].tolist() == [0x78, 0x30, 0x28, 0x01, 0x00, 0x82]     # ties go to the even code
