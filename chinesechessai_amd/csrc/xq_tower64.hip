// xq_tower64.hip — the whole convolutional trunk of a 64-channel policy/value network in ONE launch.
//
//   planes [G][10][9][16] bf16  ->  conv3x3(16->64)+ReLU  ->  nblocks x { conv+ReLU, conv+skip+ReLU }
//                               ->  1x1 heads (policy 32, value 8)+ReLU  ->  P [G][90*32], V [G][90*8]
//
// At 64 channels a layer's weights are small (a tap is 8 KB) and a board's activations are 11.25 KB: what is scarce is
// no longer LDS but LDS read bandwidth per MFMA and the cost of a workgroup barrier per step.  k_tower64 is built
// around that, not around k_tower256's split:
//
//   work split   a wave = TWO boards x ALL 64 output channels: weights on the MFMA rows (4 tiles of 16), pixels on the
//                columns (6 tiles of 16 per board, 96 columns for 90 pixels): f32x4 acc[4][12] = 192 accumulator
//                registers, one wave per SIMD, 8 boards per 256-thread workgroup.  A weight fragment read from LDS
//                serves both boards: 4 + 12 = 16 ds_read_b128 per 48 MFMAs (one board per wave: 10 per 24).
//   LDS          [weight ring 4 x 8,192][head weights 48 x 128][8 boards x (90 pixel rows x 128 B + a zero row)][dump row]
//                = 132,224 B.  A board's rows are read and written by ONE wave only: a layer's epilogue overwrites the
//                rows the layer just read (its MFMAs have consumed every fragment, and a wave's LDS operations stay in
//                order), and no workgroup barrier guards activations.  The second board of a wave sits BSTRIDE behind
//                the first, zero row included, so its fragment addresses are the first board's plus an immediate.
//   skip         the residual stream of the wave's two boards stays in registers as packed bf16 in the accumulator
//                layout (lane (r, q) of tile (mt, nt): four consecutive channels of one pixel = two registers,
//                4 x 12 x 2 = 96 VGPRs); the epilogue of a block's second convolution adds them in fp32 before the
//                block's single rounding.  No second activation region, no selector MFMA.
//   K loop       a layer = 9 steps; a step = one tap = one weight stage [64 cout][64 cin] bf16 = 8,192 B = two K-steps
//                of 32 input channels x 48 v_mfma_f32_16x16x32_bf16 = 96 MFMAs per wave (864 per layer and wave, 432
//                per board).  Stage g -> ring buffer g & 3 by LDS-DMA, 8 pieces of 1 KB, two per wave; every weight
//                byte fetched from L2 serves 8 boards.  Weight fragments are double-buffered by K-step and fetched one
//                K-step ahead; an activation fragment is refetched for the next K-step right behind the 4 MFMAs that
//                consumed it.
//   step barrier one per step, behind the first pixel tile of the step's second K-step: s_waitcnt vmcnt(4) (the wave's
//                own pieces of stage g + 1 have landed; g + 2 and g + 3 may be in flight) + s_barrier.  That tile's
//                MFMAs have consumed all weight fragments of stage g, so behind the barrier buffer g & 3 is dead and
//                stage g + 4 is requested into it; stages past the end refetch the last stage into a dead buffer.
//   channel deal row i of weight tile mt is output channel (mt >> 1) * 32 + (i >> 2) * 8 + (mt & 1) * 4 + (i & 3): a
//                lane's results of tiles 2j and 2j + 1 are 8 consecutive channels = one 16-byte chunk of a pixel row
//                (ds_write_b128), chunk j * 4 + q = exactly the fragment (K-step j, lane quarter q) of the next
//                layer.  Chunk c of pixel p sits at position c ^ (p & 7); LDS row rho of a weight stage holds the
//                dealt channel's 64 input channels, chunk c at position c ^ (rho & 7) (swizzled on the DMA source).
//   input conv   w1 [9][64][16] = 18,432 B over the ring, the planes in the tail of each board's rows; K-step = 2 taps
//                x 16 planes, 5 K-steps, the tenth tap reads the zero row.
//   heads        wh's 48 real rows are staged once beside the ring; per board 3 row tiles x 6 pixel tiles x 2 K-steps.
//   order        every output element is accumulated by one wave in one fixed order (bias, taps 0..8, K-steps 0..1,
//                skip) that depends neither on G nor on the board's place in the launch: same planes -> same bits.
//                Boards at or beyond *n_rows: a workgroup without a row returns before any barrier or DMA; a missing
//                board of a live workgroup computes on zero planes and stores nothing.
// The pixel permutation and dead-tap elimination of the 128-channel asm kernel are not here: padding MFMAs stay.
// Reference ops: neural_network.py:47-71,172-187 with eval-mode BatchNorm folded.
#include "../../include/xq_selfplay.h"
#include "xq_mfma.hpp"
#include "xq_tower_args.hpp"
#include <type_traits>

namespace {
using namespace xqm;

constexpr int PIX = 90, CH = 64, NB = 8;          // NB boards per workgroup, two per wave
constexpr int ROW = CH * 2;                       // one pixel's activations, bytes
constexpr int STAGE = CH * ROW;                   // one weight stage [64 cout][64 cin] bf16: 8,192
constexpr int HEADS = 4 * STAGE, HEAD_BYTES = 48 * ROW;
constexpr int ACT0 = HEADS + HEAD_BYTES;
constexpr int ZREL = PIX * ROW;                   // a board's zero row, behind its 90 pixel rows
constexpr int BSTRIDE = ZREL + ROW;               // 11,648
constexpr int PLREL = ZREL - PIX * 32;            // the planes [90][16] bf16 in the tail of the board's rows
constexpr int DUMP = ACT0 + NB * BSTRIDE;          // where the epilogue's lanes of the 6 slots past pixel 89 store (never read)
constexpr int LDS_BYTES64 = DUMP + ROW;
constexpr int TILE = 16 * ROW;                    // a pixel tile's rows: the ds_read immediate of tile t is t * TILE
static_assert(LDS_BYTES64 == 132224 && LDS_BYTES64 <= 163840, "LDS plan");
static_assert(9 * CH * 32 <= 4 * STAGE && ACT0 % ROW == 0 && BSTRIDE % ROW == 0, "w1 fits the ring; rows stay 128-byte aligned");
static_assert(5 * TILE + BSTRIDE + 127 < 65536, "fragment immediates fit ds_read's 16-bit offset");

__global__ __launch_bounds__(256) void k_tower64(TowerArgs A)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int nrows = A.G;
    if (A.n_rows) { const int n = *A.n_rows; nrows = n < A.G ? n : A.G; }
    if ((int)blockIdx.x * NB >= nrows) return;     // compaction: no row for this workgroup (uniform, before any barrier / DMA)
    const int board0 = blockIdx.x * NB + wave * 2;
    const int act_off = ACT0 + wave * 2 * BSTRIDE;
    const int r16 = lane & 15, q = lane >> 4;
    // row i of weight tile mt -> output channel (see "channel deal" above); chan4: the lane's four accumulator rows
    auto chan_row = [&](int mt, int i) { return (mt >> 1) * 32 + (i >> 2) * 8 + (mt & 1) * 4 + (i & 3); };
    auto chan4 = [&](int mt) { return (mt >> 1) * 32 + q * 8 + (mt & 1) * 4; };
    const int nlayers = 2 * A.nblocks, nstages = nlayers * 9;

    f32x4 acc[4][12];                                                 // [weight tile][board * 6 + pixel tile]
    uint32_t sk[4][12][2];                                            // the residual stream, packed bf16, same layout

    // ---------------------------------------------------------------- staging: zero rows, w1, head weights, planes
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    if (lane < 16) lds_st128(act_off + (lane >> 3) * BSTRIDE + ZREL + (lane & 7) * 16, zero4);
#pragma unroll
    for (int j = 0; j < 5; j++) {                                     // w1: 18 pieces of 1 KB, unswizzled [9][64][16]
        const int piece = j * 4 + wave;
        if (piece < 18) dma16_abs(reinterpret_cast<const uint8_t *>(A.w1) + piece * 1024 + lane * 16, piece * 1024);
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {                                     // wh rows 0..47: 6 pieces, chunk c of row rho at c ^ (rho & 7)
        const int piece = j * 4 + wave;
        if (piece < 6)
            dma16_abs(reinterpret_cast<const uint8_t *>(A.wh) + (piece * 8 + (lane >> 3)) * ROW + (((lane & 7) ^ (lane >> 3)) << 4),
                      HEADS + piece * 1024);
    }
#pragma unroll
    for (int bb = 0; bb < 2; bb++) {                                  // 180 chunks of 16 B per board
        const int board = board0 + bb, pl = act_off + bb * BSTRIDE + PLREL;
        if (board < nrows) {
            const int srow = A.row_src ? A.row_src[board] : board;   // (wave-uniform: a scalar load)
            const uint8_t *src = reinterpret_cast<const uint8_t *>(A.planes) + (size_t)srow * PIX * 32;
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (j * 64 + lane < PIX * 2) dma16_abs(src + (j * 64 + lane) * 16, pl + j * 1024);
        } else {
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (j * 64 + lane < PIX * 2) lds_st128(pl + (j * 64 + lane) * 16, zero4);
        }
    }
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {                                  // the accumulators start at this layer's bias
        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(A.bias + chan4(mt));
#pragma unroll
        for (int nt = 0; nt < 12; nt++) acc[mt][nt] = b4;
    }
    barrier_dma();

    // ---------------------------------------------------------------- input conv (16 -> 64)
    {
        uint32_t vm[2] = { 0, 0 };        // tap validity of the 6 pixels of this lane, 9 bits each
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const int o = nt * 16 + r16;
            uint32_t m = 0;
            if (o < PIX) {
                const int yy = o / 9, xx = o % 9;
#pragma unroll
                for (int t = 0; t < 9; t++) {
                    const int dy = t / 3 - 1, dx = t % 3 - 1;
                    if (yy + dy >= 0 && yy + dy < 10 && xx + dx >= 0 && xx + dx < 9) m |= 1u << t;
                }
            }
            vm[nt / 3] |= m << ((nt % 3) * 9);
        }
#pragma unroll
        for (int pair = 0; pair < 5; pair++) {                       // K-step = taps (2 pair, 2 pair + 1) x 16 planes
            const int tap = 2 * pair + (q >> 1);
            const bool tap_real = tap < 9;
            const int tp = tap_real ? tap : 8;
            const int off = (tp / 3 - 1) * 9 + (tp % 3 - 1);
            bf16x8 bf[12], af[4];
#pragma unroll
            for (int nt = 0; nt < 6; nt++) {
                const bool ok = tap_real && ((vm[nt / 3] >> ((nt % 3) * 9 + tp)) & 1u);
                const int sp = nt * 16 + r16 + off;
                const int a = act_off + (ok ? PLREL + sp * 32 : ZREL + (sp & 3) * 32) + (q & 1) * 16;
                bf[nt] = lds_ld128(a);
                bf[nt + 6] = lds_ld128(a + BSTRIDE);
            }
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
                af[mt] = lds_ld128((tp * CH + chan_row(mt, r16)) * 32 + (q & 1) * 16);
#pragma unroll
            for (int nt = 0; nt < 12; nt++)
#pragma unroll
                for (int mt = 0; mt < 4; mt++)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt], bf[nt], acc[mt][nt], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    barrier_dma();                                                 // every wave is done with the tap slices in the ring

    // ---------------------------------------------------------------- weight stream of the 64-channel layers
    // stage g = (layer, tap) -> ring buffer g & 3 as 64 rows of 128 B.  LDS row rho = P * 8 + (lane >> 3) of piece P
    // holds channel chan_row(P >> 1, (P & 1) * 8 + (lane >> 3)): a scalar row offset per piece plus a lane part; the
    // 16-byte chunk at position c of row rho is source chunk c ^ (rho & 7)
    const rsrc_t wrsrc = make_rsrc(A.wt, nstages * STAGE);
    const int wsrc = ((lane >> 5) * 8 + ((lane >> 3) & 3)) * ROW + (((lane & 7) ^ (lane >> 3)) << 4);
    auto stage_dma = [&](int g) {                                     // (past the end: the last stage again, into a dead buffer)
        const int gg = g < nstages ? g : nstages - 1;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int P = wave * 2 + j;
            dma16_buf_abs(wrsrc, wsrc, gg * STAGE + ((P >> 2) * 32 + (P & 1) * 16 + ((P >> 1) & 1) * 4) * ROW,
                          (g & 3) * STAGE + P * 1024);
        }
    };
    // A fragment (weight tile mt, K-step ks) of the stage at ring offset wb: ((abase + wb) ^ (ks << 6)) + mt * 2048
    const int abase = r16 * ROW + ((q ^ (r16 & 7)) << 4);
    auto load_a = [&](bf16x8 &af, int mt, int aw, int ks) { af = lds_ld128((aw ^ (ks << 6)) + mt * TILE); };

    // row validity as lane masks (wave-uniform): pixel tile t, lane -> pixel t * 16 + r16.
    // Only tile 0 holds board row 0, only tile 5 holds board row 9 and the 6 slots past pixel 89.
    bool xl[6], xr[6];
#pragma unroll
    for (int t = 0; t < 6; t++) {
        const int p = t * 16 + r16, xx = p % 9;
        xl[t] = xx != 0 && p < PIX;
        xr[t] = xx != 8 && p < PIX;
    }
    const bool real5 = r16 < PIX - 80, yu0 = r16 >= 9, yd5 = r16 == 0;
    // row address of (pixel tile t, tap) of the wave's first board, before the K-step term and without t * TILE:
    //   real pixel : act_off + sp * 128 + slot,  sp = r16 + tap offset (tile-independent: 16 | t * 16)
    //   padding    : the board's zero row at the slot the lane's own row would have used
    const int Rrow = act_off + r16 * ROW, r5 = r16 << 4, q4 = q << 4;
    auto tap_addrs = [&](int (&as)[6], int tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1, off = dy * 9 + dx;
        // (an opaque copy of the row base per call keeps the tap's address arithmetic where it is written: hoisted out
        // of the layer loop the 54 addresses would compete with the accumulators and the skip for registers)
        int rrow = Rrow, r5o = r5;
        asm volatile("" : "+v"(rrow), "+v"(r5o));
        const int slot = ((r5o + off * 16) & 0x70) ^ q4;              // (q ^ (sp & 7)) << 4
        const int aok = rrow + off * ROW + slot;
#pragma unroll
        for (int t = 0; t < 6; t++) {
            const bool sel = dx != 0 || (t == 0 && dy < 0) || t == 5;
            if (!sel) { as[t] = aok; continue; }
            bool ok = dx < 0 ? xl[t] : dx > 0 ? xr[t] : real5;      // (dx == 0 needs a select for tile 5 and for tile 0 / row 0)
            if (dx == 0 && t == 0) ok = yu0;
            else if (t == 0 && dy < 0) ok = ok && yu0;
            if (t == 5 && dy > 0) ok = ok && yd5;
            as[t] = ok ? aok : slot + (act_off + ZREL - t * TILE);
        }
    };
    // (act_off, ZREL, BSTRIDE and TILE are multiples of 128: the low 7 bits of an address are its slot, the K-step an XOR)
    auto load_b = [&](bf16x8 &bf, const int (&as)[6], int n, int ks) {
        bf = lds_ld128((as[n % 6] ^ (ks << 6)) + (n % 6) * TILE + (n / 6) * BSTRIDE);
    };

    // epilogue of one layer: acc (bias inside) [+ skip] -> bf16 -> ReLU -> the wave's own LDS rows in place; the
    // accumulators restart at the next layer's bias.  MODE 0: first convolution of a block; 1: second (adds the skip
    // registers in fp32 and keeps its output as the next block's skip); 2: input convolution (keeps its output)
    const int sbase = act_off + abase;                                // chunk q of pixel r16 (+ t * TILE, ^ (j << 6): K-step j)
    auto epilogue = [&](auto mode, const f32x4 (&bn)[4]) {
        constexpr int MODE = decltype(mode)::value;
        int s5[2];                                                    // tile 5 of either board: a select, not a branch
#pragma unroll
        for (int bb = 0; bb < 2; bb++) s5[bb] = r16 < PIX - 80 ? sbase + 5 * TILE + bb * BSTRIDE : DUMP + q4;
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int nt = 0; nt < 12; nt++) {
                f32x4 v0 = acc[2 * j][nt], v1 = acc[2 * j + 1][nt];
                if constexpr (MODE == 1) {
                    v0[0] += bf16_lo(sk[2 * j][nt][0]); v0[1] += bf16_hi(sk[2 * j][nt][0]);
                    v0[2] += bf16_lo(sk[2 * j][nt][1]); v0[3] += bf16_hi(sk[2 * j][nt][1]);
                    v1[0] += bf16_lo(sk[2 * j + 1][nt][0]); v1[1] += bf16_hi(sk[2 * j + 1][nt][0]);
                    v1[2] += bf16_lo(sk[2 * j + 1][nt][1]); v1[3] += bf16_hi(sk[2 * j + 1][nt][1]);
                }
                const uint4 pk = make_uint4(relu_bf16x2(pack_bf16x2(v0[0], v0[1])), relu_bf16x2(pack_bf16x2(v0[2], v0[3])),
                                            relu_bf16x2(pack_bf16x2(v1[0], v1[1])), relu_bf16x2(pack_bf16x2(v1[2], v1[3])));
                if constexpr (MODE != 0) {
                    sk[2 * j][nt][0] = pk.x; sk[2 * j][nt][1] = pk.y;
                    sk[2 * j + 1][nt][0] = pk.z; sk[2 * j + 1][nt][1] = pk.w;
                }
                acc[2 * j][nt] = bn[2 * j];
                acc[2 * j + 1][nt] = bn[2 * j + 1];
                if (nt % 6 < 5) lds_st128((sbase ^ (j << 6)) + (nt % 6) * TILE + (nt / 6) * BSTRIDE, pk);
                else lds_st128(s5[nt / 6] ^ (j << 6), pk);
                __builtin_amdgcn_sched_barrier(0);                    // (one tile pair at a time: nothing to gain from mixing them)
            }
    };
    auto load_bias = [&](f32x4 (&bn)[4], int row) {
#pragma unroll
        for (int mt = 0; mt < 4; mt++) bn[mt] = *reinterpret_cast<const f32x4 *>(A.bias + row * CH + chan4(mt));
    };
    using mode0 = std::integral_constant<int, 0>;
    using mode1 = std::integral_constant<int, 1>;
    using mode2 = std::integral_constant<int, 2>;

    {
        f32x4 bn[4];
        load_bias(bn, nlayers > 0 ? 1 : 0);
        if (nstages > 0) {
#pragma unroll
            for (int g = 0; g < 4; g++) stage_dma(g);
        }
        epilogue(mode2{}, bn);                                        // conv1 output; tower layer 0 starts at bias[1]
    }
    barrier_dma();                                                 // stages 0..3 have landed

    // ---------------------------------------------------------------- residual tower
    bf16x8 fa[2][4], fb[12];                                          // weight fragments by K-step parity; activation fragments
    if (nstages > 0) {
#pragma unroll
        for (int mt = 0; mt < 4; mt++) load_a(fa[0][mt], mt, abase, 0);
    }
    for (int layer = 0; layer < nlayers; layer++) {
        f32x4 bn[4];                                                  // bias of tower layer L + 1 (row L + 2; the last layer's is not used)
        load_bias(bn, layer + 2 <= nlayers ? layer + 2 : layer + 1);
        int as[6];
        tap_addrs(as, 0);
#pragma unroll
        for (int n = 0; n < 12; n++) load_b(fb[n], as, n, 0);
        const int g0 = layer * 9;
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            int asn[6];
            const int g = g0 + tap;
            const int awc = abase + ((g & 3) << 13), awn = abase + (((g + 1) & 3) << 13);
#pragma unroll
            for (int ks = 0; ks < 2; ks++) {
                const bool last = tap == 8 && ks == 1;                // last K-step of the layer: no activation prefetch
                if (ks == 1 && !last) tap_addrs(asn, tap + 1);
#pragma unroll
                for (int n = 0; n < 12; n++) {                        // (board, pixel tile) n: 4 MFMAs
#pragma unroll
                    for (int mt = 0; mt < 4; mt++)
                        acc[mt][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[ks][mt], fb[n], acc[mt][n], 0, 0, 0);
                    // this tile's activation fragment of the next K-step
                    if (!last) {
                        if (ks == 0) load_b(fb[n], as, n, 1);
                        else load_b(fb[n], asn, n, 0);
                    }
                    // the next K-step's weight fragments (ks == 1: from the stage the barrier just published)
                    if (ks == 0 && n < 4) load_a(fa[1][n], n, awc, 1);
                    if (ks == 1 && n >= 1 && n < 5) load_a(fa[0][n - 1], n - 1, awn, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (ks == 1 && n == 0) {
                        // step barrier: stage g + 1 has landed (every wave drains its own pieces first) and, this tile's
                        // MFMAs having consumed all 4 weight fragments of stage g's second K-step, nobody reads buffer
                        // g & 3 any more: stage g + 4 goes there
                        __builtin_amdgcn_s_waitcnt(0x0F74);           // vmcnt(4)
                        __builtin_amdgcn_s_barrier();
                        __builtin_amdgcn_sched_barrier(0);
                        stage_dma(g + 4);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if (tap < 8) {
#pragma unroll
                for (int t = 0; t < 6; t++) as[t] = asn[t];
            }
        }
        if (layer & 1) epilogue(mode1{}, bn);
        else epilogue(mode0{}, bn);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                               // vmcnt(0): no DMA piece is in flight when the wave ends

    // ---------------------------------------------------------------- heads (1x1, 64 -> 32 + 8)
    // per board: head rows 0..15 and 16..31 (policy), 32..47 (value channels 32..39 and 8 zero rows) x 6 pixel tiles
    // (the lane's coordinates again from a fresh lane id, not CSE-able with the tower's: nothing of the heads' address
    // arithmetic stays live across the tower, where accumulators, skip and fragments take the register file)
    int ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    const int hr = ln & 15, hq = ln >> 4;
    const int habase = hr * ROW + ((hq ^ (hr & 7)) << 4), hsbase = act_off + habase;
    bf16x8 ha[3][2];
#pragma unroll
    for (int mt = 0; mt < 3; mt++)
#pragma unroll
        for (int ks = 0; ks < 2; ks++) ha[mt][ks] = lds_ld128(HEADS + mt * TILE + (habase ^ (ks << 6)));
#pragma unroll
    for (int bb = 0; bb < 2; bb++) {
        const int board = board0 + bb;
        if (board >= nrows) break;                                    // (wave-uniform; no barrier follows)
        f32x4 hacc[3][6];
#pragma unroll
        for (int mt = 0; mt < 3; mt++)
#pragma unroll
            for (int t = 0; t < 6; t++)
#pragma unroll
                for (int i = 0; i < 4; i++) hacc[mt][t][i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int t = 0; t < 6; t++) {
                const int a = (t < 5 || hr < PIX - 80) ? hsbase + t * TILE : act_off + ZREL + (hq << 4);
                const bf16x8 hb = lds_ld128((a ^ (ks << 6)) + bb * BSTRIDE);
#pragma unroll
                for (int mt = 0; mt < 3; mt++)
                    hacc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha[mt][ks], hb, hacc[mt][t], 0, 0, 0);
            }
        uint8_t *Pb = reinterpret_cast<uint8_t *>(A.P) + (size_t)board * PIX * 64;
        uint8_t *Vb = reinterpret_cast<uint8_t *>(A.V) + (size_t)board * PIX * 16;
#pragma unroll
        for (int mt = 0; mt < 3; mt++) {
            const int c0 = mt * 16 + 4 * hq;                         // head channel of element 0
            const f32x4 b4 = *reinterpret_cast<const f32x4 *>(A.bh + c0);
#pragma unroll
            for (int t = 0; t < 6; t++) {
                const int p = t * 16 + hr;
                if (p < PIX && (mt < 2 || hq < 2)) {                 // value head: channels 32..39 only
                    const float v0 = hacc[mt][t][0] + b4[0], v1 = hacc[mt][t][1] + b4[1];
                    const float v2 = hacc[mt][t][2] + b4[2], v3 = hacc[mt][t][3] + b4[3];
                    const uint2 pk = make_uint2(relu_bf16x2(pack_bf16x2(v0, v1)), relu_bf16x2(pack_bf16x2(v2, v3)));
                    if (mt < 2) *reinterpret_cast<uint2 *>(Pb + p * 64 + c0 * 2) = pk;
                    else *reinterpret_cast<uint2 *>(Vb + p * 16 + (c0 - 32) * 2) = pk;
                }
            }
        }
    }
}

}  // namespace

extern "C" int xq_tower64_nhwc_bf16(void *stream, const void *planes, const void *w1, const void *wt, const void *bias,
                                    const void *wh, const void *bh, void *policy_out, void *value_out, int n_boards,
                                    int n_blocks, const void *row_src_dev, const void *n_rows_dev)
{
    if (!planes || !w1 || !bias || !wh || !bh || !policy_out || !value_out || n_boards <= 0 || n_blocks < 0 ||
        (n_blocks > 0 && !wt) || n_blocks > 64)
        return XQ_E_INVALID;
    TowerArgs a{ (const uint16_t *)planes, (const uint16_t *)w1, (const uint16_t *)wt, (const float *)bias,
                 (const uint16_t *)wh, (const float *)bh, (uint16_t *)policy_out, (uint16_t *)value_out, n_boards, n_blocks,
                 nullptr, (const int32_t *)row_src_dev, (const int32_t *)n_rows_dev };
    if (int rc = tower_lds_opt_in<&k_tower64>(LDS_BYTES64)) return rc;
    hipLaunchKernelGGL(k_tower64, dim3((n_boards + NB - 1) / NB), dim3(256), LDS_BYTES64, reinterpret_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : XQ_E_HIP;
}
