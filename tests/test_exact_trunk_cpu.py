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


# ---------------------------------------------------------------------------------------------------------------------
# The MXFP8 cases of tests/test_gpu_trunk_exact_mx.py

MX_CASES = [(c,) + case for c in (128, 256) for case in X.mx_cases(c)]
MX_TOWER_CASES = [case for case in MX_CASES if case[1] > 0]
# what test_trunk*_mx_against_float64_chain's bound (old_bound) accepts on these networks, as measured on the CPU: these
# two mutants in every case, every other mutant in none (their largest error is 1.03 to 6,463 times the bound)
MX_OLD_BOUND_ACCEPTS = {X.MX_PLUS_ONE_AT_BOUNDARY, X.MX_FLUSH}


@functools.lru_cache(maxsize=None)
def _mx_case(channels, blocks, k, jmax, G):
    t = X.integer_net_mx(channels, blocks, k, jmax, X.mx_net_seed(channels, blocks, k, jmax))
    planes = X.cpu_planes(G, X.PLANES_SEED)
    last = {}
    return t, planes, X.mx_chain(t, planes, blocks, last_layer_input=last), last


def test_integer_net_mx_is_what_it_says():
    from chinesechessai_amd.neural_network import mx_dequantize
    t, base = X.integer_net_mx(128, 2, 24, 3, 3), X.integer_net(128, 2, 24, 3)
    assert t.wq.shape == (4, 9, 128, 128) and t.wscale.shape == (4, 9, 128, 4) and t.wq.dtype == t.wscale.dtype == torch.uint8
    for name in ("w1", "bias", "wh", "bh"):
        assert torch.equal(getattr(t, name), getattr(base, name))
    w = mx_dequantize(t.wq, t.wscale).view(4, 9, 128, 4, 32)
    ratio = w / base.wt.double().view(4, 9, 128, 4, 32)             # nan where the integer weight is zero
    assert set(ratio[~ratio.isnan()].unique().tolist()) == {1.0, 2.0, 4.0, 8.0}
    live = ~ratio.isnan()
    assert (torch.where(live, ratio, ratio.nan_to_num(0).amax(-1, keepdim=True)) == ratio.nan_to_num(0).amax(-1, keepdim=True)).all()
    assert torch.equal(w == 0, base.wt.double().view(4, 9, 128, 4, 32) == 0)
    # the scale byte of a block whose largest weight is 2^j is j - 8 + 127; an all-zero block has 127
    assert set(t.wscale.unique().tolist()) <= {119, 120, 121, 122, 127} and len(t.wscale.unique()) >= 4
    empty = X.integer_net_mx(256, 0, 0, 0, 0)
    assert empty.wq.shape == (0, 9, 256, 256) and empty.wscale.shape == (0, 9, 256, 8)


def test_mx_activation_on_known_values():
    """One block each; the scale puts the maximum into [256, 512), e4m3 then steps by 32 from 256 and by 2^-9 below 2^-6."""
    def q(values, **kw):
        x = torch.zeros(32, dtype=torch.float64)
        x[:len(values)] = torch.tensor(values, dtype=torch.float64)
        return X.mx_activation(x, **kw)[:len(values)].tolist()
    # maximum 28 = 1.75 * 16 is the boundary: scale 2^-4, 28 -> 448; 17 -> 272 is a tie between 256 and 288, 19 -> 304
    # one between 288 and 320; with the +1 fired nothing here changes (e4m3 is floating point), so the values are equal
    assert q([28, 17, 19, 21, 3]) == [28, 16, 20, 20, 3]
    assert q([28, 17, 19, 21, 3], mutant=X.MX_PLUS_ONE_AT_BOUNDARY) == [28, 16, 20, 20, 3]
    assert q([28, 17, 19, 21, 3], mutant=X.MX_TRUNCATE) == [28, 16, 18, 20, 3]
    assert q([28, 17, 19, 21, 3], mutant=X.MX_TIES_AWAY) == [28, 18, 20, 22, 3]
    # maximum 29 > 1.75 * 16: the +1 fires, 29 -> 232 is a tie between 224 and 240; without it 29 -> 464, a tie between
    # 448 and 480, and 31 -> 496 -> 480 saturates to 448 = 28
    assert q([29, 31 - 2]) == [28, 28] and q([31, 30]) == [32, 30]
    assert q([31, 30], mutant=X.MX_NO_PLUS_ONE) == [28, 28]
    # maximum 2^15 -> 256 (scale 2^7): 1 -> 2^-7 is subnormal (step 2^-9 = a quarter unit: kept), 3 -> 3 * 2^-7 is normal;
    # the flush mutant loses the 1
    assert q([32768, 1, 3]) == [32768, 1, 3] and q([32768, 1, 3], mutant=X.MX_FLUSH) == [32768, 0, 3]
    # maximum 2^18 -> 256 (scale 2^10): the subnormal step is 2 units: 1 is a tie and goes to 0, 3 to 4, 5 to 4, 7 to 8
    assert q([262144, 1, 3, 5, 7, 9]) == [262144, 0, 4, 4, 8, 8]
    # maximum 1.75 * 2^17 at the boundary (scale 2^9, subnormal step 1); one scale step more and the step is 2 units
    assert q([229376, 1, 3, 5]) == [229376, 1, 3, 5]
    assert q([229376, 1, 3, 5], mutant=X.MX_PLUS_ONE_AT_BOUNDARY) == [229376, 0, 4, 4]
    stats = {k: 0 for k in ("plus_one", "at_boundary", "changed", "ties", "subnormal", "flushed", "boundary_lossy")}
    stats["act_scales"] = set()
    X.mx_activation(torch.tensor([229376.0, 1, 3, 5] + [0.0] * 60, dtype=torch.float64), stats=stats)
    assert stats == {"plus_one": 0, "at_boundary": 1, "changed": 0, "ties": 0, "subnormal": 3, "flushed": 0,
                     "boundary_lossy": 3, "act_scales": {127 + 9}}
    # the neighbour's scale byte: block 0 (scale 2^-4) comes back under block 1's (2^-3) and the other way round
    two = torch.tensor([28.0] + [0.0] * 31 + [56.0] + [0.0] * 31, dtype=torch.float64)
    assert X.mx_activation(two, swap_scales=True)[[0, 32]].tolist() == [56, 28]


@pytest.mark.parametrize("channels,blocks,k,jmax,G", MX_CASES)
def test_mx_headroom_and_quantiser_events(channels, blocks, k, jmax, G):
    """Every case of the MXFP8 GPU module on CPU planes of the same density: headroom below 2^23 (X.MX_EXACT: measured,
    below the 2^24 of the fp32 significand), head outputs that vary, and from one block up the quantiser's events - 100
    blocks where the +1 fired, 100 at mantissa exactly 1.75, 1,000 e4m3 ties, 1,000 changed values, 4 activation scale
    bytes; 4 weight scale bytes with jmax = 3; 1,000 subnormals in (6, 5, 1) and (20, 2, 0); in (6, 5, 1) an element that
    a +1 at 1.75 would change (X.mx_assert_reached; the dense block's one-board run is asked for its share of the blocks,
    the runs from the middle count up for the whole thresholds, here once more)."""
    t, planes, ch, last = _mx_case(channels, blocks, k, jmax, G)
    print("C=%d blocks=%d k=%s jmax=%d G=%d: headroom 2^%.2f, +1 in %d blocks, %d at 1.75, %d values changed, %d ties, %d "
          "subnormal (%d to zero), %d / %d activation / weight scale bytes, %d lossy at the boundary, %d distinct outputs" % (
              channels, blocks, "dense" if k == X.DENSE else k, jmax, G, math.log2(ch.headroom), ch.plus_one, ch.at_boundary,
              ch.changed, ch.ties, ch.subnormal, ch.flushed, ch.act_scales, ch.w_scales, ch.boundary_lossy,
              len(ch.bits.unique())))
    assert ch.bits.shape == (G, 90, 40)
    X.mx_assert_reached(ch, channels, blocks, k, jmax, G)
    if blocks == 0:
        assert ch[2:] == (0,) * 9                                    # no tower: nothing is quantised
        assert torch.equal(ch.bits, X.float64_chain(X.integer_net(channels, 0, 0, X.NET_SEED), planes, 0).bits)
    elif G >= X.BOARDS[channels][1]:
        assert min(ch.plus_one, ch.at_boundary) >= 100 and min(ch.ties, ch.changed) >= 1000 and ch.act_scales >= 4


@pytest.mark.parametrize("channels,blocks,k,jmax,G", MX_CASES)
def test_mx_float32_chain_equals_float64_chain(channels, blocks, k, jmax, G):
    t, planes, ch, last = _mx_case(channels, blocks, k, jmax, G)
    c32 = X.mx_chain(t, planes, blocks, dtype=torch.float32)
    assert X.first_difference(c32.bits, ch.bits) is None, X.first_difference(c32.bits, ch.bits)
    assert c32[1:] == ch[1:]


@pytest.mark.parametrize("channels,blocks,k,jmax,G", MX_TOWER_CASES)
def test_mx_mutants_change_a_bit(channels, blocks, k, jmax, G):
    """Eight wrong quantisers or scale routings.  Truncation, ties away, the missing +1, the fp32 sum and both misrouted
    scale bytes change a head bit in every case with a tower; flushed subnormals in the cases that assert subnormals.
    The +1 at exactly 1.75 changes a head bit in (6, 5, 1) at both widths (X.MX_BOUNDARY_CASES, where the 256-channel net
    has a seed of its own for it) and equals the right rule wherever boundary_lossy is 0 (asserted: no test can tell it
    apart there).  With each: its max-norm error against the bound of test_trunk*_mx_against_float64_chain, asserted as
    measured (MX_OLD_BOUND_ACCEPTS): a statement about that test, not a tolerance of this one.  The two mutants of the
    last tower layer start from the right chain's input to that layer."""
    t, planes, ch, last = _mx_case(channels, blocks, k, jmax, G)
    ref = ch.bits.view(torch.bfloat16).double()
    bound = X.old_bound(ch.bits, blocks)
    for name in X.MX_MUTANTS:
        m = X.mx_chain(t, planes, blocks, mutant=name, last_layer_input=last).bits
        if name in X.MX_LAST_LAYER_MUTANTS and G == 1:              # the short cut, once per width against the whole chain
            assert last and torch.equal(m, X.mx_chain(t, planes, blocks, mutant=name).bits)
        differ = int((m != ch.bits).sum())
        err =(m.view(torch.bfloat16).double() - ref).abs().max().item()
        print("C=%d blocks=%d k=%d jmax=%d G=%d mutant %-70s %6d outputs differ, max-norm error / old bound = %.4f" % (
            channels, blocks, k, jmax, G, name + ":", differ, err / bound))
        if name == X.MX_PLUS_ONE_AT_BOUNDARY:
            if (blocks, k, jmax) in X.MX_BOUNDARY_CASES:
                assert differ > 0, name
            assert ch.boundary_lossy > 0 or differ == 0
        elif name == X.MX_FLUSH:
            if (blocks, k, jmax) in X.MX_SUBNORMAL_CASES:
                assert differ > 0, name
            assert ch.subnormal > 0 or differ == 0
        else:
            assert differ > 0, name
        assert (err <= bound) == (name in MX_OLD_BOUND_ACCEPTS), name
