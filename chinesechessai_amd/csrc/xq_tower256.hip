// xq_tower256.hip — the whole convolutional trunk of a 256-channel policy/value network in ONE launch.
//
//   planes [G][10][9][16] bf16  ->  conv3x3(16->256)+ReLU  ->  nblocks x { conv+ReLU, conv+skip+ReLU }
//                               ->  1x1 heads (policy 32, value 8)+ReLU  ->  P [G][90*32], V [G][90*8]
//
// The 128-channel kernels of xq_tower.hip cannot be stretched: at 256 channels a board's activations are 46 KB, a
// [256 cout][64 cin] weight stage is 32 KB and the input convolution's nine tap slices are 72 KB.  k_tower256 keeps
// k_tower16b's MFMA shape, wave tile and issue style and changes the split around them:
//
//   work split   a wave = (board, 64-channel QUARTER of the output channels): wave tile 96 pixels x 64 channels =
//                f32x4 acc[4][6], 96 accumulator registers.  4 waves per board, 2 boards per 512-thread workgroup,
//                one workgroup per CU, two waves per SIMD.
//   LDS          [weight stages 2 x 32,768][activations 2 boards x 46,080][zero row 512][bias 2 x 1,024 f32]
//                = 160,256 B of the CU's 163,840.  Activations stay here from the planes to the heads; a layer's
//                output overwrites its input rows.
//   K loop       a layer = 9 taps x 8 K-steps of 32 input channels = 36 weight stages [256 cout][64 cin] of two
//                K-steps each, one stream per workgroup for both boards: 32 LDS-DMA pieces of 1 KB per stage, 4 per
//                wave, stage g -> buffer g & 1, refilled two stages ahead.  Per wave and layer 9 x 8 x 24 = 1,728
//                v_mfma_f32_16x16x32_bf16 (6,912 per board; the 128-channel layer has 1,728 per board).  The tap
//                loop is fully unrolled so that every s_waitcnt lgkmcnt is an exact count; activation fragments are
//                double-buffered by K-step, weight fragments are fetched one K-step ahead.
//   stage barrier  raw s_barrier + vmcnt(0) behind the first pixel tile of a stage's second K-step: its 4 MFMAs have
//                consumed all 4 weight fragments of the retiring buffer, so every wave's reads of it are complete
//                when it arrives, and each wave's own DMA pieces of the next stage have landed.
//   in-place epilogue  the last stage barrier of a layer also waits lgkmcnt(0): all 8 waves (both boards: they share
//                the barrier because they share the weight stream) have every activation read of the layer behind
//                them before any wave stores.
//   channel deal the output channels are dealt to the MFMA rows so that a lane's results of weight tiles 2j and
//                2j + 1 are 8 consecutive channels = one 16-byte chunk of a 512-byte activation row: the epilogue
//                stores ds_write_b128.  Chunk (K-step ks, lane quarter q) of pixel p sits at
//                ((q & 1) << 4 | ks << 1 | q >> 1) ^ (p & 7).
//   skip         as in k_tower16b: the first convolution of a block re-reads the block input x (the wave's own 64
//                channels = two K-steps) from the rows it is about to overwrite and starts the second convolution's
//                accumulators at x + bias = S . X + bias through the matrix pipe (S a 0/1 selector): the skip is
//                added in fp32 before the block's single bf16 rounding.  Every bias enters as an accumulator start.
//   input conv   w1 [9][256][16] = 73,728 B is staged at once over both weight buffers and the first 8 KB of board
//                0's activation region (free then: the planes sit in the TAIL of each board's region); K-step = 2 taps
//                x 16 planes, 5 K-steps, the tenth tap reads the zero row.
//   heads        wh [64][256] into weight buffer 0; K = 256 in 8 K-steps; of a board's 4 waves one takes policy rows
//                0..15, one 16..31, one the value rows, one idles (48 MFMAs per wave).
//   order        every output element is accumulated by one wave in one fixed order (bias, taps 0..8, K-steps 0..7)
//                that depends neither on G nor on the board's place in the launch or the workgroup: same planes ->
//                same bits.  Boards at or beyond *n_rows: their workgroups return before any barrier or DMA; the empty
//                second slot of the last workgroup computes on whatever its LDS holds and stores nothing.
// The pixel permutation and dead-tap elimination of the 128-channel asm kernel are not here: padding MFMAs stay.
// Reference ops: neural_network.py:47-71,172-187 with eval-mode BatchNorm folded.
#include "../../include/xq_selfplay.h"
#include "xq_mfma.hpp"
#include "xq_tower_args.hpp"
#include <type_traits>

namespace {
using namespace xqm;

constexpr int PIX = 90, CH = 256;
constexpr int ROW = CH * 2;                       // one pixel's activations, bytes
constexpr int ACT_BYTES = PIX * ROW;              // one board: 46,080
constexpr int WBUF_BYTES = CH * 128;              // one weight stage [256 cout][64 cin] bf16: 32,768
constexpr int ACT0 = 2 * WBUF_BYTES, ZROW = ACT0 + 2 * ACT_BYTES, BIAS = ZROW + ROW;     // bias: [2][256] f32
constexpr int LDS_BYTES256 = BIAS + 2 * CH * 4;   // 160,256
constexpr int TILE = 16 * ROW;                    // a pixel tile's rows: the ds_read immediate of tile nt is nt * TILE
constexpr int SPL = 36;                           // weight stages per layer
static_assert(LDS_BYTES256 == 160256 && LDS_BYTES256 <= 163840, "LDS plan");
static_assert(9 * CH * 32 <= ACT0 + ACT_BYTES - PIX * 32, "the input convolution's tap slices must end before board 0's planes");

__global__ __launch_bounds__(512, 2) void k_tower256(TowerArgs A)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wb_ = wave >> 2, qc = wave & 3;                         // board in workgroup, channel quarter
    // row i of weight tile mt -> output channel (see "channel deal" above)
    auto chan_row = [&](int mt, int i) { return qc * 64 + (mt >> 1) * 32 + (i >> 2) * 8 + (mt & 1) * 4 + (i & 3); };
    int nrows = A.G;
    if (A.n_rows) { const int n = *A.n_rows; nrows = n < A.G ? n : A.G; }
    if ((int)blockIdx.x * 2 >= nrows) return;      // compaction: no row for this workgroup (uniform, before any barrier / DMA)
    const int board = blockIdx.x * 2 + wb_;
    const bool board_ok = board < nrows;
    const int act_off = ACT0 + wb_ * ACT_BYTES;
    const int r16 = lane & 15, q = lane >> 4;

    f32x4 acc[4][6];

    // ---------------------------------------------------------------- input conv (16 -> 256)
    const int pl_off = act_off + ACT_BYTES - PIX * 32;                // planes [90][16] bf16 in the tail of the board's region
    if (tid < 32) lds_st128(ZROW + tid * 16, make_uint4(0, 0, 0, 0));
    const int nlayers = 2 * A.nblocks, nstages = nlayers * SPL;
    if (wave == 1 && nstages > 0) dma16_abs(A.bias + CH + lane * 4, BIAS + CH * 4);          // bias[1] -> slot 1
#pragma unroll
    for (int j = 0; j < 9; j++) {                                     // w1: 72 pieces of 1 KB, unswizzled [9][256][16]
        const int piece = j * 8 + wave;
        dma16_abs(reinterpret_cast<const uint8_t *>(A.w1) + piece * 1024 + lane * 16, piece * 1024);
    }
    if (board_ok && qc < 3) {                                         // 180 chunks of 16 B: three waves of the board
        const int srow = A.row_src ? A.row_src[board] : board;      // (wave-uniform: a scalar load)
        const uint8_t *src = reinterpret_cast<const uint8_t *>(A.planes) + (size_t)srow * PIX * 32;
        const int idx = qc * 64 + lane;
        if (idx < PIX * 2) dma16_abs(src + idx * 16, pl_off + qc * 1024);
    }
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {                                  // the accumulators start at this layer's bias
        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(A.bias + chan_row(mt, 4 * q));
#pragma unroll
        for (int nt = 0; nt < 6; nt++) acc[mt][nt] = b4;
    }
    barrier_dma();
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
            bf16x8 bf[6], af[4];
#pragma unroll
            for (int nt = 0; nt < 6; nt++) {
                const bool ok = tap_real && ((vm[nt / 3] >> ((nt % 3) * 9 + tp)) & 1u);
                const int sp = nt * 16 + r16 + off;
                bf[nt] = lds_ld128((ok ? pl_off + sp * 32 : ZROW + (sp & 7) * 32) + (q & 1) * 16);
            }
#pragma unroll
            for (int mt = 0; mt < 4; mt++)
                af[mt] = lds_ld128((tp * CH + chan_row(mt, r16)) * 32 + (q & 1) * 16);
#pragma unroll
            for (int nt = 0; nt < 6; nt++)
#pragma unroll
                for (int mt = 0; mt < 4; mt++)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt], bf[nt], acc[mt][nt], 0, 0, 0);
        }
    }
    barrier_dma();                                                 // every wave is done with planes and tap slices
                                                                   // (its MFMAs consumed them: no LDS read is in flight)

    // ---------------------------------------------------------------- weight stream of the 256-channel layers
    // stage g = (layer, tap, K-slice g & 3): [256 cout][64 cin] -> buffer g & 1 as 256 rows of 128 B.  LDS row
    // rho = piece * 8 + (lane >> 3) holds the weights of channel chan_row(rho) (quarter piece >> 3, weight tile
    // (piece >> 1) & 3, tile rows (piece & 1) * 8 ..): a scalar row offset per piece plus a lane part; the 16-byte
    // chunk at position c of row rho is source chunk c ^ ((rho >> 1) & 7)
    const rsrc_t wrsrc = make_rsrc(A.wt, nlayers * 9 * CH * CH * 2);
    const int wch = (lane & 7) ^ (lane >> 4);
    const int wsrc_even = ((lane >> 5) * 8 + ((lane >> 3) & 3)) * ROW + (wch << 4), wsrc_odd = wsrc_even ^ 64;
    auto piece_off = [&](int P) { return ((P >> 3) * 64 + ((P >> 2) & 1) * 32 + (P & 1) * 16 + ((P >> 1) & 1) * 4) * ROW; };
    auto stage_piece = [&](int g, int buf, int j) {                   // j < 4
        const int soff = (g >> 2) * (CH * CH * 2) + (g & 3) * 128 + piece_off(wave * 4 + j);
        dma16_buf_abs(wrsrc, (j & 1) ? wsrc_odd : wsrc_even, soff, buf * WBUF_BYTES + (wave * 4 + j) * 1024);
    };
    // A fragment (weight tile mt, K-step kk of a stage): abase ^ (kk << 6), + mt * 2048
    const int abase = (qc * 64 + r16) * 128 + ((q ^ ((r16 >> 1) & 7)) << 4);
    auto load_a1 = [&](bf16x8 &af, int mt, int buf, int kk) {
        af = lds_ld128((abase ^ (kk << 6)) + buf * WBUF_BYTES + mt * 2048);
    };

    // row validity as lane masks (wave-uniform): pixel tile nt, lane -> pixel nt * 16 + r16.
    // Only tile 0 holds board row 0, only tile 5 holds board row 9 and the 6 slots past pixel 89.
    bool xl[6], xr[6];
#pragma unroll
    for (int nt = 0; nt < 6; nt++) {
        const int p = nt * 16 + r16, xx = p % 9;
        xl[nt] = xx != 0 && p < PIX;
        xr[nt] = xx != 8 && p < PIX;
    }
    const bool real5 = r16 < PIX - 80, yu0 = r16 >= 9, yd5 = r16 == 0;
    // row address of (pixel tile nt, tap), before the K-step term and without nt * TILE (ds_read immediate):
    //   real pixel : act_off + sp * 512 + slot,  sp = r16 + tap offset (tile-independent: 16 | nt * 16)
    //   padding    : the zero row at the slot the lane's own row would have used
    const int Rrow = act_off + r16 * ROW, r5 = r16 << 4, q4 = (((q & 1) << 4) | (q >> 1)) << 4;
    auto tap_addrs = [&](int (&as)[6], int tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1, off = dy * 9 + dx;
        // (an opaque copy of the row base per call keeps the tap's address arithmetic where it is written: hoisted
        // out of the layer loop the 54 addresses would be spilled)
        int rrow = Rrow, r5o = r5;
        asm volatile("" : "+v"(rrow), "+v"(r5o));
        const int slot = ((r5o + off * 16) & 0x70) ^ q4;              // (((q & 1) << 4 | q >> 1) ^ (sp & 7)) << 4
        const int aok = rrow + off * ROW + slot;
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const bool sel = dx != 0 || (nt == 0 && dy < 0) || nt == 5;
            if (!sel) { as[nt] = aok; continue; }
            bool ok = dx < 0 ? xl[nt] : dx > 0 ? xr[nt] : real5;    // (dx == 0 needs a select for tile 5 and for tile 0 / row 0)
            if (dx == 0 && nt == 0) ok = yu0;
            else if (nt == 0 && dy < 0) ok = ok && yu0;
            if (nt == 5 && dy > 0) ok = ok && yd5;
            as[nt] = ok ? aok : slot + (ZROW - nt * TILE);
        }
    };
    // (act_off, ZROW and TILE are multiples of 512: the low 9 bits of an address are its slot, the K-step is an XOR)
    auto load_b1 = [&](bf16x8 &bf, int a, int nt, int ks) { bf = lds_ld128((a ^ (ks << 5)) + nt * TILE); };

    // epilogue of one layer: acc (bias [+ skip] already inside) -> bf16 -> ReLU -> LDS rows in place;
    // READ_X (first convolution of a block): the block input x is read back from those rows first and
    // the next layer's accumulators start at x + bias; otherwise they start at the next layer's bias
    auto epilogue = [&](auto read_x, int lb_next) {
        int ln;                                                       // lane id again, not CSE-able with the loop's
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        const int r = ln & 15, qq = ln >> 4;
        int sb[6];                                                    // this lane's chunk of K-step qc * 2 (+ j: ^ (j << 5)) of pixel nt * 16 + r
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const int p = nt * 16 + r < PIX ? nt * 16 + r : 0;
            sb[nt] = act_off + p * ROW + ((((((qq & 1) << 4) | (qq >> 1)) ^ (qc << 2)) ^ (p & 7)) << 4);
        }
        const int lbq = lb_next + (qc * 64 + qq * 8) * 4;              // bias of channel qc * 64 + j * 32 + qq * 8 + t * 4 ..
        // x + bias = S . X + bias: row i of selector tile 2j + t picks input channel (i >> 2) * 8 + t * 4 + (i & 3) of
        // K-step qc * 2 + j, X = this wave's own 64 channels of the block input as 12 ordinary B fragments, bias as the
        // C operand: one fp32 addition per element (exact products, the MFMA adder's rounding)
        bf16x8 xf[2][6], sel[2];
        if constexpr (decltype(read_x)::value) {
#pragma unroll
            for (int k2 = 0; k2 < 2; k2++)
#pragma unroll
                for (int nt = 0; nt < 6; nt++) xf[k2][nt] = lds_ld128(sb[nt] ^ (k2 << 5));     // the chunk this lane overwrites below
#pragma unroll
            for (int o = 0; o < 2; o++)
#pragma unroll
                for (int j = 0; j < 8; j++)
                    sel[o][j] = (qq == (r >> 2) && j == o * 4 + (r & 3)) ? (__bf16)1.0f : (__bf16)0.0f;
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const f32x4 bn0 = lds_ldf4(lbq + j * 128), bn1 = lds_ldf4(lbq + j * 128 + 16);
#pragma unroll
            for (int nt = 0; nt < 6; nt++) {
                const f32x4 v0 = acc[2 * j][nt], v1 = acc[2 * j + 1][nt];
                const uint4 pk = make_uint4(relu_bf16x2(pack_bf16x2(v0[0], v0[1])), relu_bf16x2(pack_bf16x2(v0[2], v0[3])),
                                            relu_bf16x2(pack_bf16x2(v1[0], v1[1])), relu_bf16x2(pack_bf16x2(v1[2], v1[3])));
                if constexpr (decltype(read_x)::value) {
                    acc[2 * j][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sel[0], xf[j][nt], bn0, 0, 0, 0);
                    acc[2 * j + 1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sel[1], xf[j][nt], bn1, 0, 0, 0);
                } else {
                    acc[2 * j][nt] = bn0;
                    acc[2 * j + 1][nt] = bn1;
                }
                if (nt < 5 || r < PIX - 80) lds_st128(sb[nt] ^ (j << 5), pk);
            }
        }
    };
    using yes = std::integral_constant<bool, true>;
    using no = std::integral_constant<bool, false>;

    if (nstages > 0) {
#pragma unroll
        for (int j = 0; j < 4; j++) { stage_piece(0, 0, j); stage_piece(1, 1, j); }
    }
    epilogue(no{}, BIAS + CH * 4);                                  // conv1 output; tower layer 0 starts at bias[1]
    barrier_dma();

    // ---------------------------------------------------------------- residual tower
    bf16x8 fa[2][4], fb[2][6];                                       // fragments, double-buffered by K-step parity
    if (nstages > 0) {
#pragma unroll
        for (int mt = 0; mt < 4; mt++) load_a1(fa[0][mt], mt, 0, 0);
    }
    for (int layer = 0; layer < nlayers; layer++) {
        if (wave == 1 && layer + 1 < nlayers)                       // bias of tower layer L + 1 (row L + 2) -> slot L & 1
            dma16_abs(A.bias + (size_t)(layer + 2) * CH + lane * 4, BIAS + (layer & 1) * CH * 4);
        int as[6];
        tap_addrs(as, 0);
#pragma unroll
        for (int nt = 0; nt < 6; nt++) load_b1(fb[0][nt], as[nt], nt, 0);
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            int asn[6];
#pragma unroll
            for (int ks = 0; ks < 8; ks++) {                        // 8 K-steps of 32 channels = 4 weight stages
                const int buf = (ks >> 1) & 1, kk = ks & 1, cur = ks & 1;
                const int g = layer * SPL + tap * 4 + (ks >> 1);
                const bool last = tap == 8 && ks == 7;                // last K-step of the layer: no activation prefetch
                if (ks == 7 && !last) tap_addrs(asn, tap + 1);
#pragma unroll
                for (int n = 0; n < 6; n++) {                        // pixel tile n: 4 MFMAs
                    // the next K-step's activation fragment of this tile
                    if (!last) {
                        if (ks < 7) load_b1(fb[cur ^ 1][n], as[n], n, ks + 1);
                        else load_b1(fb[cur ^ 1][n], asn[n], n, 0);
                    }
                    // the next K-step's weight fragments (kk == 1: from the stage the barrier just published)
                    // and the refill of the retiring buffer two stages ahead (the last two stages of the tower
                    // refetch the final stage into a dead buffer rather than branch)
                    if (kk == 0 && n < 4) load_a1(fa[cur ^ 1][n], n, buf, 1);
                    if (kk == 1 && n >= 1 && n < 5) {
                        load_a1(fa[cur ^ 1][n - 1], n - 1, buf ^ 1, 0);
                        stage_piece(g + 2 < nstages ? g + 2 : nstages - 1, buf, n - 1);
                    }
#pragma unroll
                    for (int mt = 0; mt < 4; mt++)
                        acc[mt][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[cur][mt], fb[cur][n], acc[mt][n], 0, 0, 0);
                    // issue order inside the tile: one filler (fragment read, DMA piece) per MFMA gap
                    const int nrd = (last ? 0 : 1) + ((kk == 0 && n < 4) || (kk == 1 && n >= 1 && n < 5) ? 1 : 0);
                    if (nrd >= 1) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (nrd == 2) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if (kk == 1 && n >= 1 && n < 5) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                    if (kk == 1 && n == 0) {
                        // stage barrier: the next stage has landed (every wave drains its own pieces first) and, this
                        // tile's MFMAs having consumed all 4 weight fragments of buffer buf, nobody reads it any more
                        __builtin_amdgcn_sched_barrier(0);
                        if (last) __builtin_amdgcn_s_waitcnt(0x0070);      // vmcnt(0) lgkmcnt(0): + all activation reads done
                        else __builtin_amdgcn_s_waitcnt(0x0F70);           // vmcnt(0)
                        __builtin_amdgcn_s_barrier();
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if (tap < 8) {
#pragma unroll
                for (int nt = 0; nt < 6; nt++) as[nt] = asn[nt];
            }
        }
        if (layer & 1) epilogue(no{}, BIAS + (layer & 1) * CH * 4);
        else epilogue(yes{}, BIAS + (layer & 1) * CH * 4);
        barrier_dma();
    }

    // ---------------------------------------------------------------- heads (1x1, 256 -> 32 + 8)
    {
        const uint8_t *src = reinterpret_cast<const uint8_t *>(A.wh);     // [64][512 B] -> buffer 0, chunk ^ ((row & 7) << 1)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int q0 = (wave * 4 + j) * 64, idx = q0 + lane, row = idx >> 5, cp = idx & 31;
            dma16_abs(src + row * ROW + ((cp ^ ((row & 7) << 1)) * 16), q0 * 16);
        }
    }
    f32x4 hacc[6];
#pragma unroll
    for (int nt = 0; nt < 6; nt++)
#pragma unroll
        for (int i = 0; i < 4; i++) hacc[nt][i] = 0.f;
    barrier_dma();
    if (!board_ok || qc == 3) return;                                // (no barrier follows)
    // wave qc of a board: head rows qc * 16 .. + 16 (0, 1: policy channels; 2: value channels 32..39 and 8 zero rows)
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {
        bf16x8 hb[6];
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const int p = nt * 16 + r16 < PIX ? nt * 16 + r16 : 0;
            hb[nt] = lds_ld128(act_off + p * ROW + (((((q & 1) << 4) | (ks << 1) | (q >> 1)) ^ (p & 7)) << 4));
        }
        const int row = qc * 16 + r16;
        const bf16x8 ha = lds_ld128(row * ROW + (((ks * 4 + q) ^ ((row & 7) << 1)) << 4));
#pragma unroll
        for (int nt = 0; nt < 6; nt++)
            hacc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha, hb[nt], hacc[nt], 0, 0, 0);
    }
    uint8_t *Pb = reinterpret_cast<uint8_t *>(A.P) + (size_t)board * PIX * 64;
    uint8_t *Vb = reinterpret_cast<uint8_t *>(A.V) + (size_t)board * PIX * 16;
    const int c0 = qc * 16 + 4 * q;                                  // head channel of element 0
    const f32x4 b4 = *reinterpret_cast<const f32x4 *>(A.bh + c0);
#pragma unroll
    for (int nt = 0; nt < 6; nt++) {
        const int p = nt * 16 + r16;
        if (p < PIX && (qc < 2 || q < 2)) {                          // value head: channels 32..39 only
            const float v0 = hacc[nt][0] + b4[0], v1 = hacc[nt][1] + b4[1];
            const float v2 = hacc[nt][2] + b4[2], v3 = hacc[nt][3] + b4[3];
            const uint2 pk = make_uint2(relu_bf16x2(pack_bf16x2(v0, v1)), relu_bf16x2(pack_bf16x2(v2, v3)));
            if (qc < 2) *reinterpret_cast<uint2 *>(Pb + p * 64 + c0 * 2) = pk;
            else *reinterpret_cast<uint2 *>(Vb + p * 16 + (c0 - 32) * 2) = pk;
        }
    }
}

}  // namespace

extern "C" int xq_tower256_nhwc_bf16(void *stream, const void *planes, const void *w1, const void *wt, const void *bias,
                                     const void *wh, const void *bh, void *policy_out, void *value_out, int n_boards,
                                     int n_blocks, const void *row_src_dev, const void *n_rows_dev)
{
    if (!planes || !w1 || !bias || !wh || !bh || !policy_out || !value_out || n_boards <= 0 || n_blocks < 0 ||
        (n_blocks > 0 && !wt) || n_blocks > 64)
        return XQ_E_INVALID;
    TowerArgs a{ (const uint16_t *)planes, (const uint16_t *)w1, (const uint16_t *)wt, (const float *)bias,
                 (const uint16_t *)wh, (const float *)bh, (uint16_t *)policy_out, (uint16_t *)value_out, n_boards, n_blocks,
                 nullptr, (const int32_t *)row_src_dev, (const int32_t *)n_rows_dev };
    if (int rc = tower_lds_opt_in<&k_tower256>(LDS_BYTES256)) return rc;
    hipLaunchKernelGGL(k_tower256, dim3((n_boards + 1) / 2), dim3(512), LDS_BYTES256, reinterpret_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : XQ_E_HIP;
}
