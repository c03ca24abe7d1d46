"""The integer networks of tests/exact_trunk.py, checked on the CPU for everything tests/test_gpu_trunk_exact.py relies
on: the headroom that makes fp32 accumulation exact in any order, enough roundings and exact ties for a wrong rounding
to show, mutants of the chain that must each change an output bit, and the chain in float32 against itself in float64."""
import functools
import math

import pytest
import torch

from tests import exact_trunk as X

CASES = [(c,) + case for c in (64, 128, 192, 256) for case in X.trunk_cases(c)]
MUTANTS = (("truncation", {"round_fn": X.truncate}), ("ties away from zero", {"round_fn": X.ties_away}),
           ("skip after the rounding", {"skip_before_rounding": False}), ("tap 0 dropped", {"drop_tap0": True}))


@functools.lru_cache(maxsize=None)
def _case(channels, blocks, k, G):
    t = X.integer_net(channels, blocks, k, X.NET_SEED)
    planes = X.cpu_planes(G, X.PLANES_SEED)
    return t, planes, X.float64_chain(t, planes, blocks)


def test_integer_net_is_what_it_says():
    t = X.integer_net(64, 2, 24, 3)
    assert t.w1.shape == (9, 64, 16) and t.wt.shape == (4, 9, 64, 64) and t.bias.shape == (5, 64)
    assert t.wh.shape == (64, 64) and t.bh.shape == (64,)
    assert t.w1.dtype == t.wt.dtype == t.wh.dtype == torch.bfloat16 and t.bias.dtype == t.bh.dtype == torch.float32
    assert (t.w1[..., 15] == 0).all() and t.w1.abs().max() == 2 and t.bias.abs().max() == 2
    assert set(t.wt.double().unique().tolist()) == {-1.0, 0.0, 1.0}
    assert (t.wt.double().abs().sum(dim=(1, 3)) == 24).all()               # per (layer, cout): 24 weights over (tap, cin)
    assert (t.wh[:40].double().abs().sum(1) == 8).all() and (t.wh[40:] == 0).all() and (t.bh[40:] == 0).all()
    d = X.integer_net(64, 1, X.DENSE, 3).wt.double()
    assert d.shape == (2, 9, 64, 64) and 0.6 < d.abs().mean().item() < 0.72 and abs(d.mean().item()) < 0.01
    for a, b in zip(t, X.integer_net(64, 2, 24, 3)):
        assert torch.equal(a, b)


def test_rounding_functions_on_known_values():
    # bf16 steps by 2 from 256 and by 8 from 1024: 257, 259, 261 and 1028 are exact ties, 1029 is above one
    x = torch.tensor([256.0, 257.0, 258.0, 259.0, 261.0, 1028.0, 1029.0, -257.0, -259.0, 3.0, 0.0], dtype=torch.float64)
    assert X.rne(x).tolist() == [256, 256, 258, 260, 260, 1024, 1032, -256, -260, 3, 0]
    assert X.truncate(x).tolist() == [256, 256, 258, 258, 260, 1024, 1024, -256, -258, 3, 0]
    assert X.ties_away(x).tolist() == [256, 258, 258, 260, 262, 1032, 1032, -258, -260, 3, 0]


@pytest.mark.parametrize("channels,blocks,k,G", CASES)
def test_headroom_and_something_to_round(channels, blocks, k, G):
    """Every case of the GPU module, on CPU planes of the same density (the GPU module asserts the headroom again on the
    planes it launches with).  2^24 is derived, not measured: fp32 has a 24-bit significand, so sums of integers whose
    magnitudes add up to less are exact in any order.  A case within a factor 4 of it would get a smaller k."""
    t, planes, ch = _case(channels, blocks, k, G)
    bits = ch.bits
    nonzero = (bits != 0).double().mean().item()
    distinct = len(bits.unique())
    print("C=%d blocks=%d k=%s G=%d: headroom 2^%.1f, %d roundings changed a value, %d exact ties, %.0f %% of head outputs "
          "non-zero, %d distinct" % (channels, blocks, "dense" if k == X.DENSE else k, G, math.log2(ch.headroom), ch.changed,
                                     ch.ties, 100 * nonzero, distinct))
    assert ch.headroom < X.EXACT
    assert bits.shape == (G, 90, 40) and nonzero > 0.3
    if blocks == 0:
        # the stem and the heads alone: every sum of |terms| is below 256, the first integer spacing of bf16 above 1, so
        # no rounding can change a value and the outputs cannot take 100 values; what is left to ask is that they vary
        assert ch.headroom < 256 and ch.changed == 0 and ch.ties == 0 and distinct > 10
    else:
        assert ch.changed >= 100 and ch.ties >= 20 and distinct > 100


@pytest.mark.parametrize("channels", (64, 128, 192, 256))
@pytest.mark.parametrize("blocks,k", ((1, X.DENSE), (6, 6)))
def test_mutants_change_a_bit(channels, blocks, k):
    """Four wrong trunks, each of which the bit comparison must tell from the right one; printed with each: its max-norm
    error over the bound of the test_trunk*_against_float64_chain tests (DESIGN.md records which of them that bound lets
    through)."""
    t, planes, ch = _case(channels, blocks, k, X.BOARDS[channels][1])
    ref = ch.bits.view(torch.bfloat16).double()
    bound = X.old_bound(ch.bits, blocks)
    for name, kw in MUTANTS:
        m = X.float64_chain(t, planes, blocks, **kw).bits
        err = (m.view(torch.bfloat16).double() - ref).abs().max().item()
        print("C=%d blocks=%d mutant %-24s %6d outputs differ, max-norm error / old bound = %.4f (%s)" % (
            channels, blocks, name + ":", int((m != ch.bits).sum()), err / bound, "accepted" if err <= bound else "rejected"))
        assert not torch.equal(m, ch.bits), name
        assert X.first_difference(m, ch.bits).split(" of ")[0] == str(int((m != ch.bits).sum()))
    assert X.first_difference(ch.bits.clone(), ch.bits) is None


@pytest.mark.parametrize("channels,blocks,k,G", CASES)
def test_float32_chain_equals_float64_chain(channels, blocks, k, G):
    """Order independence on the host: the same chain with every convolution accumulated in float32 by the library, in
    whatever order it likes, gives the same bits, the same headroom and the same counts."""
    t, planes, ch = _case(channels, blocks, k, G)
    c32 = X.float64_chain(t, planes, blocks, dtype=torch.float32)
    assert X.first_difference(c32.bits, ch.bits) is None, X.first_difference(c32.bits, ch.bits)
    assert (c32.headroom, c32.changed, c32.ties) == (ch.headroom, ch.changed, ch.ties)
