"""Integer-valued networks on which every bf16 trunk kernel must agree with a float64 restatement in every bit.

The argument ("Bit-exact integer networks"): planes are 0/1 and every weight and bias is an integer, so every
activation is an integer; an integer rounded to bf16 is an integer again; every bf16 x bf16 product is exact in fp32, and
every partial sum, in any order, is exact while the sum of |terms| of that output stays below 2^24 (the fp32 significand).
The fp32 accumulator therefore holds the exact sum whatever the MFMA shape, K order or wave split, and the single bf16
rounding that follows is a function of an exact number.  `headroom` is that sum of |terms|, maximised over every output
of every layer; the tests assert headroom < 2^24 before they compare anything.

Plain torch on the CPU, nothing here touches a GPU."""
import collections

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
