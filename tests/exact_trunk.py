"""Integer-valued networks on which every bf16 trunk kernel must agree with a float64 restatement in every bit.

The argument ("Bit-exact integer networks"): planes are 0/1 and every weight and bias is an integer, so every
activation is an integer; an integer rounded to bf16 is an integer again; every bf16 x bf16 product is exact in fp32, and
every partial sum, in any order, is exact while the sum of |terms| of that output stays below 2^24 (the fp32 significand).
The fp32 accumulator therefore holds the exact sum whatever the MFMA shape, K order or wave split, and the single bf16
rounding that follows is a function of an exact number.  `headroom` is that sum of |terms|, maximised over every output
of every layer; the tests assert headroom < 2^24 before they compare anything.

Plain torch on the CPU, nothing here touches a GPU."""
import collections
import math

import torch
import torch.nn.functional as F

EXACT = 2 ** 24                     # fp32 holds every integer of magnitude below this, so do sums of such terms
DENSE = -1                          # k: every (tap, cin) position of every output channel is drawn from {-1, 0, 1}

IntegerNet = collections.namedtuple("IntegerNet", "w1 wt bias wh bh")
Chain = collections.namedtuple("Chain", "bits headroom changed ties")

# (blocks, k) of every trunk kernel's depth cases; the dense block has 9 * C weights per output channel, the deeper nets
# fewer (the activations grow by about the square root of k per layer): 20 blocks of 3 weights reach 2^24 at 256 channels
DEPTHS = ((0, 0), (1, DENSE), (2, 24), (6, 6), (20, 2))
# board counts per kernel: one board, one board into a second and a third workgroup (8 / 3 / 2 boards per workgroup for
# k_tower64 / k_tower192 / k_tower256 and build 36 of the 128-channel kernel, 4 for build 39)
BOARDS = {64: (1, 9, 17), 128: (1, 5, 9), 192: (1, 4, 7), 256: (1, 3, 5)}
NET_SEED, PLANES_SEED = 0, 5


def trunk_cases(channels):
    """(blocks, k, G) of one trunk kernel: the dense block at all three board counts, every other depth at the middle one."""
    lo, mid, hi = BOARDS[channels]
    out = []
    for blocks, k in DEPTHS:
        out += [(blocks, k, g) for g in ((lo, mid, hi) if k == DENSE else (mid,))]
    return out


def integer_net(channels, blocks, k, seed):
    """The tensors the C entries read, every value an integer: w1 [9][C][16] bf16 in -2..2 (input channel 15 zero),
    wt [2 * blocks][9][C][C] bf16 ([layer][tap][cout][cin]) with k weights of +-1 per output channel at random (tap, cin)
    positions (k = DENSE: every position from {-1, 0, 1}), bias [1 + 2 * blocks][C] fp32 in -2..2, wh [64][C] bf16 with 8
    weights of +-1 in each of the 40 head rows and rows 40..63 zero, bh [64] fp32 in -2..2 (rows 40..63 zero)."""
    C = channels
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randint(-2, 3, (9, C, 16), generator=g).double()
    w1[..., 15] = 0

    def sparse(rows, cols, n):                          # n entries of +-1 at distinct random columns of every row
        pos = torch.rand(rows, cols, generator=g).topk(n, dim=1).indices
        sign = torch.randint(0, 2, (rows, n), generator=g).double() * 2 - 1
        return torch.zeros(rows, cols, dtype=torch.float64).scatter_(1, pos, sign)
    if k == DENSE or k == 9 * C:
        wt = torch.randint(-1, 2, (2 * blocks, 9, C, C), generator=g).double()
    else:
        # [layer][cout][tap * C + cin] -> [layer][tap][cout][cin]
        wt = torch.stack([sparse(C, 9 * C, k).view(C, 9, C).permute(1, 0, 2) for _ in range(2 * blocks)]) if blocks else \
            torch.zeros(0, 9, C, C, dtype=torch.float64)
    bias = torch.randint(-2, 3, (1 + 2 * blocks, C), generator=g).float()
    wh = torch.zeros(64, C, dtype=torch.float64)
    wh[:40] = sparse(40, C, 8)
    bh = torch.zeros(64)
    bh[:40] = torch.randint(-2, 3, (40,), generator=g).float()
    return IntegerNet(w1.bfloat16().contiguous(), wt.bfloat16().contiguous(), bias.contiguous(), wh.bfloat16().contiguous(), bh)


def cpu_planes(G, seed):
    """[G][10][9][16] bf16 planes of 0 / 1 at the density of the GPU tests' generator (15 %), plane 15 zero."""
    g = torch.Generator().manual_seed(seed)
    planes = torch.zeros(G, 10, 9, 16, dtype=torch.bfloat16)
    planes[..., :15] = (torch.rand(G, 10, 9, 15, generator=g) < 0.15).to(torch.bfloat16)
    return planes


def _f32_bits(x):
    f = x.float()
    assert torch.equal(f.to(x.dtype), x), "a value that fp32 does not hold: the headroom is gone"
    return f.contiguous().view(torch.int32)


def rne(x):
    """bf16, round to nearest, ties to even: what v_cvt_pk_bf16_f32 does."""
    return x.bfloat16().to(x.dtype)


def truncate(x):
    """bf16 by dropping the low 16 bits of the fp32 (towards zero)."""
    return (_f32_bits(x) & -65536).view(torch.float32).to(x.dtype)


def ties_away(x):
    """bf16, round to nearest, ties away from zero: add half an ulp to the magnitude, drop the low bits."""
    return ((_f32_bits(x) + 0x8000) & -65536).view(torch.float32).to(x.dtype)


def float64_chain(t, planes, blocks, round_fn=rne, skip_before_rounding=True, drop_tap0=False, dtype=torch.float64):
    """The trunk restated with F.conv2d (padding 1) in `dtype`: conv + bias, ReLU, one rounding to bf16 per layer; the
    block's skip joins the fp32 sum before the block's single rounding; the heads are one product sum + bias, ReLU, one
    rounding.  Returns Chain(bits, headroom, changed, ties): the head activations as int16 bit patterns [G, 90, 40]
    (policy 0..31, value 32..39; a zero is +0), the largest sum of |terms| over every output of every layer
    (conv2d(|x|, |w|) + |bias| + |skip|, heads included), how many roundings changed a value and how many of the rounded
    values lay exactly half way between two bf16.

    skip_before_rounding=False is the order of the per-layer path (per_layer_chain).  drop_tap0 is a mutant for the
    tests' self-check: the last tower layer loses the product of tap 0 with input pixel (0, 0), which belongs to output
    pixel (1, 1) (at output pixel (0, 0) itself tap 0 reads padding and has nothing to lose)."""
    C = t.w1.shape[1]
    stats = {"headroom": 0.0, "changed": 0, "ties": 0}

    def kernel(w):                                      # [9][cout][cin] -> [cout][cin][3][3]
        return w.to(dtype).reshape(3, 3, w.shape[1], -1).permute(2, 3, 0, 1)

    def room(v):
        stats["headroom"] = max(stats["headroom"], v.max().item())

    def rnd(x):
        stats["changed"] += int((rne(x) != x).sum())
        stats["ties"] += int(((_f32_bits(x) & 0xFFFF) == 0x8000).sum())
        return round_fn(x)

    def conv(x, w, b, skip=None, drop=False):
        y = F.conv2d(x, kernel(w), b.to(dtype), padding=1)
        r = F.conv2d(x.abs(), kernel(w).abs(), b.to(dtype).abs(), padding=1)
        if drop:
            y[:, :, 1, 1] -= x[:, :, 0, 0] @ w[0].to(dtype).t()
        room(r if skip is None else r + skip.abs())
        return y
    a = rnd(torch.relu(conv(planes.to(dtype).permute(0, 3, 1, 2), t.w1, t.bias[0])))
    for i in range(blocks):
        y = rnd(torch.relu(conv(a, t.wt[2 * i], t.bias[1 + 2 * i])))
        z = conv(y, t.wt[2 * i + 1], t.bias[2 + 2 * i], skip=a, drop=drop_tap0 and i == blocks - 1)
        a = rnd(torch.relu(z + a)) if skip_before_rounding else rnd(torch.relu(rnd(z) + a))
    x = a.permute(0, 2, 3, 1).reshape(-1, 90, C)
    room(x.abs() @ t.wh[:40].to(dtype).abs().t() + t.bh[:40].to(dtype).abs())
    h = rnd(torch.relu(x @ t.wh[:40].to(dtype).t() + t.bh[:40].to(dtype))) + 0.0        # + 0.0: a zero is +0
    return Chain(h.bfloat16().contiguous().view(torch.int16), stats["headroom"], stats["changed"], stats["ties"])


def per_layer_chain(t, planes, blocks, **kw):
    """The order of the per-layer path (xq_conv3x3_nhwc_bf16 per convolution, then xq_heads_nhwc_bf16).  The epilogue of
    k_conv3x3_b (csrc/xq_conv.hip) rounds conv + bias to bf16 into LDS ("acc + b4", pack_bf16x2: the lines under
    "epilogue: +bias -> bf16") and applies the ReLU there only when the layer has no residual (early_relu = relu && !res);
    with a residual the way out reads that bf16 back, adds the residual in fp32, rounds a second time and applies the ReLU
    last ("bf16_lo(wv[k]) + bf16_lo(rv[k])", pack_bf16x2, relu_bf16x2); lines 242-246 and 266-272 of the file when this
    was written.  So the second convolution of a block is
    relu(rne(rne(conv + bias) + skip)): two roundings where the single-launch trunk has one."""
    return float64_chain(t, planes, blocks, skip_before_rounding=False, **kw)


def old_bound(ref_bits, blocks):
    """The bound of the test_trunk*_against_float64_chain tests for these head activations."""
    ref = ref_bits.view(torch.bfloat16).double()
    return 2 ** -8 * max(1.0, ref.abs().max().item()) * (2 + blocks)


def first_difference(got, ref):
    """None when two [G, 90, 40] int16 tensors hold the same bits, else a message with the count of differing outputs and
    the first (board, pixel, channel) with both bit patterns."""
    if torch.equal(got, ref):
        return None
    d = (got != ref).nonzero()
    b, p, c = d[0].tolist()
    return "%d of %d outputs differ; first at board %d pixel %d channel %d: kernel 0x%04x, chain 0x%04x" % (
        len(d), ref.numel(), b, p, c, got[b, p, c].item() & 0xFFFF, ref[b, p, c].item() & 0xFFFF)


# ---------------------------------------------------------------------------------------------------------------------
# The MXFP8 trunk kernels (csrc/xq_tower_mx.hip, csrc/xq_tower256_mx.hip) on integer-valued networks.
#
# The argument carries over ("Bit-exact integer networks"): an integer quantised to e4m3 under a power-of-two
# block scale is an integer again (where the e4m3 step is below 1 the integer is kept, where it is 1 or more the result is
# a multiple of it), and a weight of the form integer x 2^j with at most 4 significant bits survives mx_quantize exactly.
# So every e4m3 x e4m3 product is an integer, every fp32 partial sum is exact in any order while the sum of |terms| stays
# below 2^24, and the bf16 rounding and the quantisation that follow are functions of an exact number: the in-kernel
# quantiser is pinned in every bit at every layer.

MxNet = collections.namedtuple("MxNet", "w1 wq wscale bias wh bh")
MxChain = collections.namedtuple("MxChain", "bits headroom plus_one at_boundary changed ties subnormal flushed "
                                            "act_scales w_scales boundary_lossy")
# (blocks, k, jmax) of both MXFP8 kernels: a tower weight block of 32 input channels is multiplied by 2^j, j in 0..jmax
# ((6, 5, 1) was (6, 6, 1) until k_tower256_mx differed from the chain there in one output of 10,800, see MX_EXACT;
# its 256-channel net has a seed of its own, see MX_NET_SEEDS)
MX_DEPTHS = ((0, 0, 0), (1, DENSE, 3), (2, 24, 3), (6, 6, 0), (6, 5, 1), (20, 2, 0))
MX_SUBNORMAL_CASES = ((6, 5, 1), (20, 2, 0))        # the cases that must reach 1,000 e4m3 subnormals
# The cases in which a "+1" that fires at mantissa exactly 1.75 must change a head bit, at both widths.  That rule equals
# the right one unless a block at 1.75 holds an element that one more scale step pushes below 2^-6 (MxChain.boundary_lossy:
# e4m3 is a floating-point format, everywhere else halving an element costs it nothing), which needs a block maximum of
# 2^14 or more beside odd elements of a few units: (6, 5, 1) has 13 to 40 such elements, no other case has one.  Whether
# one of them reaches a head output depends on the net.  At 128 channels NET_SEED does it on the CPU planes and on the
# GPU module's (2 and 3 outputs).  At 256 channels it does not (18 and 16 elements, no output), so that case has a net
# seed of its own: the first of 0..199 with which the mutant shows on both sets of planes (1 output each; with planes of
# one set alone seeds 1, 11, 15 or 4, 8, 14 would do).
MX_BOUNDARY_CASES = ((6, 5, 1),)
MX_NET_SEEDS = {(256, 6, 5, 1): 28}                 # (channels, blocks, k, jmax): every other case has NET_SEED
# The headroom under which every MXFP8 case matched its chain on an MI355X.  v_mfma_scale_f32_16x16x128_f8f6f4 does not
# always deliver the exact sum of its 128 products where fp32 could hold it: at (6, 6, 1), 256 channels, headroom 2^23.27,
# one last-layer sum of -13,312 (an earlier tap) + 393,216 - 8 (both in one instruction and one K block, the 8 from an
# e4m3 subnormal) came out at least 8 too large, the product 2^15.6 times smaller than its neighbour lost; the same
# network at 128 channels matched at 2^23.75, so the headroom is a stand-in for the spread of the products inside one
# instruction.  The largest headroom below the failure that matched is 2^22.87 ((6, 5, 1), 128 channels).  DESIGN.md §7.
MX_EXACT = 2 ** 23
MX_SEED = 9                                          # of the draw of j

# Mutants of mx_chain; each changes one thing.
MX_TRUNCATE = "e4m3 conversion by truncation"
MX_TIES_AWAY = "e4m3 ties away from zero"
MX_NO_PLUS_ONE = "no +1 rule, elements saturate at 448"
MX_PLUS_ONE_AT_BOUNDARY = "+1 rule fires at mantissa 1.75"
MX_FP32_SUM = "quantiser reads the fp32 sum"
MX_FLUSH = "e4m3 subnormals flushed to zero"
MX_WEIGHT_SCALE = "weight scale byte of K-block q ^ 1 in the last tower layer"
MX_ACT_SCALE = "activation scale byte of channel block q ^ 1 in the last tower layer"
MX_MUTANTS = (MX_TRUNCATE, MX_TIES_AWAY, MX_NO_PLUS_ONE, MX_PLUS_ONE_AT_BOUNDARY, MX_FP32_SUM, MX_FLUSH, MX_WEIGHT_SCALE,
              MX_ACT_SCALE)
MX_LAST_LAYER_MUTANTS = (MX_WEIGHT_SCALE, MX_ACT_SCALE)


def mx_cases(channels):
    """(blocks, k, jmax, G) of one MXFP8 kernel: the dense block at all three board counts (NB = 4 boards per workgroup in
    xq_tower_mx.hip, 2 in xq_tower256_mx.hip: one board into a second and into a third workgroup), every other depth at the
    middle one."""
    lo, mid, hi = BOARDS[channels]
    out = []
    for blocks, k, jmax in MX_DEPTHS:
        out += [(blocks, k, jmax, g) for g in ((lo, mid, hi) if k == DENSE else (mid,))]
    return out


def mx_net_seed(channels, blocks, k, jmax):
    """The net seed of an MXFP8 case: NET_SEED but for the cases of MX_NET_SEEDS."""
    return MX_NET_SEEDS.get((channels, blocks, k, jmax), NET_SEED)


def integer_net_mx(channels, blocks, k, jmax, seed):
    """integer_net's tensors with every tower weight block of 32 consecutive input channels, per (layer, tap, cout,
    K-block), multiplied by 2^j, j drawn from 0..jmax (seed MX_SEED), through mx_quantize: w1, wq e4m3 bytes
    [2 * blocks][9][C][C], wscale E8M0 bytes [2 * blocks][9][C][C / 32], bias, wh, bh - what the MXFP8 C entries read.
    The bytes dequantise to the integer weights exactly (+-2^j has one significant bit)."""
    from chinesechessai_amd.neural_network import mx_dequantize, mx_quantize
    C = channels
    t = integer_net(C, blocks, k, seed)
    g = torch.Generator().manual_seed(MX_SEED)
    j = torch.randint(0, jmax + 1, (2 * blocks, 9, C, C // 32), generator=g)
    wt = torch.ldexp(t.wt.double().view(2 * blocks, 9, C, C // 32, 32), j.unsqueeze(-1)).view(2 * blocks, 9, C, C)
    wq, ws = mx_quantize(wt)
    assert wq.shape == (2 * blocks, 9, C, C) and ws.shape == (2 * blocks, 9, C, C // 32)
    assert torch.equal(mx_dequantize(wq, ws), wt) and torch.equal(wt, wt.round())
    return MxNet(t.w1, wq.contiguous(), ws.contiguous(), t.bias, t.wh, t.bh)


def _swap_neighbours(x):
    """Along the last axis: element q takes the place of element q ^ 1."""
    return x.reshape(x.shape[:-1] + (x.shape[-1] // 2, 2)).flip(-1).reshape(x.shape)


def mx_activation(x, mutant=None, swap_scales=False, stats=None):
    """mx_dequantize(*mx_quantize(x)) of non-negative activations [..., C] (float64), restated so that one step of it can
    be wrong: per block of 32 consecutive channels m = the maximum, e = floor(log2 m) - 8, + 1 when m * 2^-e > 448 (the
    mantissa of m above 1.75), scale byte e + 127 (127 for an all-zero block), elements x * 2^-e rounded to nearest-even
    e4m3 (step 2^(floor(log2 y) - 3), 2^-9 below 2^-6), times 2^e.  With no mutant the result is asserted equal to
    mx_quantize's.  swap_scales: block q is scaled back by the byte of block q ^ 1.  stats: a dict whose event counts, taken
    by the right rule over the non-zero blocks whatever the mutant, are added to."""
    from chinesechessai_amd.neural_network import mx_dequantize, mx_quantize
    assert x.dtype == torch.float64 and bool((x >= 0).all())
    xb = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    m = xb.amax(-1)
    nz = m > 0
    e = torch.where(nz, torch.frexp(m)[1].to(torch.int64) - 9, torch.zeros_like(m, dtype=torch.int64))
    top = torch.ldexp(m, -e)                                         # in [256, 512): 256 x the mantissa of m
    plus = {MX_NO_PLUS_ONE: torch.zeros_like(nz), MX_PLUS_ONE_AT_BOUNDARY: top >= 448}.get(mutant, top > 448)
    byte = torch.where(nz, e + plus.to(torch.int64) + 127, torch.full_like(e, 127))
    assert 0 <= int(byte.min()) and int(byte.max()) <= 254
    y = torch.ldexp(xb, (127 - byte).unsqueeze(-1))
    step = torch.ldexp(torch.ones_like(y), (torch.frexp(y)[1].to(torch.int64) - 1).clamp(min=-6) - 3)
    r = y / step
    if mutant == MX_TRUNCATE:
        v = torch.floor(r) * step
    elif mutant == MX_TIES_AWAY:
        v = torch.floor(r + 0.5) * step
    else:
        v = torch.round(r) * step                                    # (torch.round: halves to even)
    sub = (y > 0) & (y < 2.0 ** -6)
    if mutant == MX_FLUSH:
        v = torch.where(sub, torch.zeros_like(v), v)
    if mutant == MX_NO_PLUS_ONE:
        v = v.clamp(max=448.0)
    assert float(v.max()) <= 448.0
    out = torch.ldexp(v, ((_swap_neighbours(byte) if swap_scales else byte) - 127).unsqueeze(-1)).reshape(x.shape)
    if mutant is None and not swap_scales:
        assert torch.equal(out, mx_dequantize(*mx_quantize(x)))
    if stats is not None:
        stats["plus_one"] += int((nz & (top > 448)).sum())
        stats["at_boundary"] += int((nz & (top == 448)).sum())
        stats["changed"] += int((out != x).sum())
        stats["ties"] += int(((y > 0) & (r - torch.floor(r) == 0.5)).sum())
        stats["subnormal"] += int(sub.sum())
        stats["flushed"] += int((sub & (v == 0)).sum())
        # e4m3 is a floating-point format: one scale step more costs an element a bit only where it then lies below 2^-6
        half_step = torch.ldexp(torch.ones_like(y), (torch.frexp(y)[1].to(torch.int64) - 2).clamp(min=-6) - 3)
        stats["boundary_lossy"] += int(((nz & (top == 448)).unsqueeze(-1) & (torch.round(y / 2 / half_step) * half_step * 2 != v)).sum())
        stats["act_scales"].update(byte[nz].unique().tolist())
    return out


def mx_chain(t, planes, blocks, mutant=None, dtype=torch.float64, last_layer_input=None):
    """float64_chain for the MXFP8 kernels: t is integer_net_mx's MxNet; in front of every tower convolution the
    bf16-rounded activation goes through mx_dequantize(*mx_quantize(.)) (mx_activation), the weights are mx_dequantize of
    the bytes.  Per layer: conv1 as in bf16; per block y = rne(relu(convq(a) + bias)), a = rne(relu(convq(y) + bias + a)),
    the skip a taken as the unquantised bf16 stream; the heads read that stream.  Returns MxChain: the head bit patterns
    and the headroom (on the quantised operands) as float64_chain, and the quantiser's events over all non-zero activation
    blocks that a tower convolution reads: blocks where the "+1" rule fired, blocks whose maximum has mantissa exactly
    1.75 (where it must not fire), elements whose quantisation changed the value, elements that were exact ties on the
    e4m3 grid, elements in the e4m3 subnormal range (below 2^-6 after scaling) and how many of those became zero, the
    number of distinct activation scale bytes and of distinct weight scale bytes, and (boundary_lossy) the elements of
    blocks at mantissa 1.75 that a scale byte one higher would quantise to another value - the only place where
    MX_PLUS_ONE_AT_BOUNDARY can show.  mutant: one of MX_MUTANTS; of a mutant's run only the bits mean anything (headroom
    and counts are not taken: 0).  last_layer_input: a dict that the right chain fills with what the last tower layer reads
    and that a mutant of that layer alone (MX_LAST_LAYER_MUTANTS), given the same t and planes, starts from."""
    from chinesechessai_amd.neural_network import mx_dequantize
    assert mutant is None or mutant in MX_MUTANTS
    C = t.w1.shape[1]
    stats = {"headroom": 0.0, "plus_one": 0, "at_boundary": 0, "changed": 0, "ties": 0, "subnormal": 0, "flushed": 0,
             "act_scales": set(), "boundary_lossy": 0}
    last = 2 * blocks - 1

    def kernel(w):                                      # [9][cout][cin] -> [cout][cin][3][3]
        return w.to(dtype).reshape(3, 3, w.shape[1], -1).permute(2, 3, 0, 1)

    def room(v):
        stats["headroom"] = max(stats["headroom"], v.max().item())

    def conv(x, w, b, skip=None):
        if mutant is None:                              # a mutant's headroom and counts are nobody's business: not taken
            room(F.conv2d(x.abs(), kernel(w).abs(), b.to(dtype).abs(), padding=1) + (0 if skip is None else skip.abs()))
        return F.conv2d(x, kernel(w), b.to(dtype), padding=1)

    def convq(s, a, i, skip=None):                      # s: the exact fp32 sum after the ReLU, a = rne(s)
        x = (s if mutant == MX_FP32_SUM else a).double().permute(0, 2, 3, 1)
        xq = mx_activation(x, mutant, swap_scales=mutant == MX_ACT_SCALE and i == last,
                           stats=stats if mutant is None else None)
        scale = _swap_neighbours(t.wscale[i]) if mutant == MX_WEIGHT_SCALE and i == last else t.wscale[i]
        w = mx_dequantize(t.wq[i], scale)
        # integers stay integers (a block scaled back by its neighbour's byte may not)
        assert mutant == MX_ACT_SCALE or (torch.equal(xq, xq.round()) and torch.equal(w, w.round()))
        return conv(xq.permute(0, 3, 1, 2).to(dtype), w, t.bias[1 + i], skip)
    if blocks and mutant in MX_LAST_LAYER_MUTANTS and last_layer_input:
        s1, y, a = last_layer_input["s1 y a"]           # of the right chain on the same t and planes: equal up to here
    else:
        s = torch.relu(conv(planes.to(dtype).permute(0, 3, 1, 2), t.w1, t.bias[0]))
        a = rne(s)
        for i in range(blocks):
            s1 = torch.relu(convq(s, a, 2 * i))
            y = rne(s1)
            if i == blocks - 1:
                break
            s = torch.relu(convq(s1, y, 2 * i + 1, skip=a) + a)
            a = rne(s)
        if blocks and mutant is None and last_layer_input is not None:
            last_layer_input["s1 y a"] = (s1, y, a)
    if blocks:
        s = torch.relu(convq(s1, y, last, skip=a) + a)
        a = rne(s)
    x = a.permute(0, 2, 3, 1).reshape(-1, 90, C)
    if mutant is None:
        room(x.abs() @ t.wh[:40].to(dtype).abs().t() + t.bh[:40].to(dtype).abs())
    h = rne(torch.relu(x @ t.wh[:40].to(dtype).t() + t.bh[:40].to(dtype))) + 0.0        # + 0.0: a zero is +0
    return MxChain(h.bfloat16().contiguous().view(torch.int16), stats["headroom"], stats["plus_one"], stats["at_boundary"],
                   stats["changed"], stats["ties"], stats["subnormal"], stats["flushed"], len(stats["act_scales"]),
                   len(t.wscale.unique()), stats["boundary_lossy"])


def mx_assert_reached(ch, channels, blocks, k, jmax, G):
    """What a run of a case must reach before anything is compared with it: the headroom that makes every fp32 sum exact
    and, from one block up, enough quantiser events of every kind for a wrong rule to show.  The counts are those of the
    case at its middle board count (and above); the dense block's one-board run has G / middle of the activation blocks
    and is asked for that share (at 128 channels it has 720 blocks in all, 360 of them conv1's, the only ones whose
    small maxima sit at mantissa 1.75 often: 100 such blocks cannot be reached there).  In numbers, at one board: 20 "+1"
    blocks, 20 blocks at 1.75, 200 ties and 200 changed values at 128 channels (1 board of 5), 34, 34, 334 and 334 at 256
    (1 of 3); reached there: 101, 50, 666, 5,385 and 200, 89, 1,114, 10,069."""
    share = min(1.0, G / BOARDS[channels][1])
    assert ch.headroom < MX_EXACT < EXACT, "headroom 2^%.2f" % math.log2(ch.headroom)
    if blocks == 0:
        # the stem and the heads alone: outputs are non-negative integers no larger than the headroom, which is below
        # 100, so they cannot take 100 values; what is left to ask is that they vary (as for the bf16 kernels)
        assert ch.headroom < 100 and len(ch.bits.unique()) > 10
    else:
        assert len(ch.bits.unique()) >= 100
        assert ch.plus_one >= 100 * share and ch.at_boundary >= 100 * share, ch[1:]
        assert ch.ties >= 1000 * share and ch.changed >= 1000 * share and ch.act_scales >= 4, ch[1:]
    if jmax == 3:
        assert ch.w_scales >= 4, ch[1:]
    if (blocks, k, jmax) in MX_SUBNORMAL_CASES:
        assert ch.subnormal >= 1000, ch[1:]
    if (blocks, k, jmax) in MX_BOUNDARY_CASES:
        assert ch.boundary_lossy > 0, ch[1:]
