// xq_tower192.hip — the whole convolutional trunk of a 192-channel policy/value network in ONE launch.
//
//   planes [G][10][9][16] bf16  ->  conv3x3(16->192)+ReLU  ->  nblocks x { conv+ReLU, conv+skip+ReLU }
//                               ->  1x1 heads (policy 32, value 8)+ReLU  ->  P [G][90*32], V [G][90*8]
//
// Neither sibling stretches to 192 channels: twelve 16-channel output tiles do not divide into k_tower256's four
// 64-channel quarters, and k_tower64's "a wave owns all outputs" would need 6 x 12 x 4 = 288 accumulator registers.
// A board's activations are 34,560 B, a [192 cout][64 cin] weight stage is 24,576 B: THREE boards fit beside two stages.
//
//   work split   a wave = (board, 48-channel QUARTER of the output channels): wave tile 96 pixels x 48 channels =
//                f32x4 acc[3][6], 72 accumulator registers.  4 waves per board, 3 boards per 768-thread workgroup,
//                one workgroup per CU, three waves per SIMD (168 registers each: accumulators 72, weight fragments
//                2 x 12, activation fragments 24, addresses).  (A wave = (board, 96-channel half) would halve the LDS
//                reads per MFMA, but puts 6 waves on 4 SIMDs: two SIMDs carry 2 x 1,944 MFMAs per layer against
//                3 x 972 here, a third more on the critical SIMD, so the matrix pipe decides for quarters.)
//   LDS          [weight stages 2 x 24,576][activations 3 boards x 34,560][zero row 384][bias 2 x 768 f32]
//                = 154,752 B of the CU's 163,840.  Activations stay here from the planes to the heads; a layer's
//                output overwrites its input rows.
//   K loop       a layer = 9 taps x 6 K-steps of 32 input channels = 27 weight stages [192 cout][64 cin] of two
//                K-steps each, one stream per workgroup for all three boards: 24 LDS-DMA pieces of 1 KB per stage, 2
//                per wave, stage g -> buffer g & 1, refilled two stages ahead.  27 is odd, so the loop runs over
//                BLOCKS (54 stages) with both layers written out: every buffer index stays a constant.  Per wave and
//                layer 9 x 6 x 18 = 972 v_mfma_f32_16x16x32_bf16 (3,888 per board).  The tap loop is fully unrolled so
//                that every s_waitcnt lgkmcnt is an exact count; weight fragments are double-buffered by K-step and
//                fetched one K-step ahead, an activation fragment is refetched for the next K-step right behind the
//                3 MFMAs that consumed it (the other two waves of the SIMD cover its latency).
//   stage barrier  raw s_barrier + vmcnt(0) behind the first pixel tile of a stage's second K-step: its 3 MFMAs have
//                consumed all 3 weight fragments of the retiring buffer, so every wave's reads of it are complete
//                when it arrives, and each wave's own DMA pieces of the next stage have landed.  All 12 waves share
//                it because they share the weight stream.
//   in-place epilogue  the last stage barrier of a layer also waits lgkmcnt(0): all 12 waves have every activation
//                read of the layer behind them before any wave stores.
//   channel deal row i of weight tile mt of quarter qc is output channel qc * 48 + mt * 16 + i, the natural order: a
//                lane's four results of a tile are 4 consecutive channels = 8 bytes of the 384-byte row and go out as
//                ds_write_b64 (three tiles cannot pair up into 16-byte chunks; 18 stores against 972 MFMAs).  The
//                16-byte chunk c = K-step * 4 + lane quarter (24 per row) of pixel p sits at position c ^ (p & 7):
//                the XOR stays inside a group of 8 chunks = 128 B, rows are 3 x 128 B, so 8 consecutive pixels of one
//                chunk - a ds_read_b128 of a fragment, or the epilogue's stores - cover all 8 positions of the
//                128-byte bank period.  LDS row rho of a weight stage holds channel rho's 64 input channels, chunk c
//                at position c ^ (rho & 7) (swizzled on the DMA source).
//   skip         k_tower256's way (the residual stream in registers would take 36 more): the first convolution of a
//                block re-reads the block input x (the wave's own 48 channels, 16 per weight tile) from the rows it is
//                about to overwrite and starts the second convolution's accumulators at x + bias = S . X + bias through
//                the matrix pipe (S a 0/1 selector): the skip is added in fp32 before the block's single bf16
//                rounding.  Every bias enters as an accumulator start.
//   input conv   w1 [9][192][16] = 55,296 B is staged at once over both weight buffers and the first 6 KB of board
//                0's activation region (free then: the planes sit in the TAIL of each board's region); K-step = 2 taps
//                x 16 planes, 5 K-steps, the tenth tap reads the zero row.
//   heads        wh [64][192] into weight buffer 0; K = 192 in 6 K-steps; of a board's 4 waves one takes policy rows
//                0..15, one 16..31, one the value rows, one idles (36 MFMAs per wave).
//   order        every output element is accumulated by one wave in one fixed order (bias, taps 0..8, K-steps 0..5)
//                that depends neither on G nor on the board's place in the launch or the workgroup: same planes ->
//                same bits.  Boards at or beyond *n_rows: their workgroups return before any barrier or DMA; an empty
//                slot of the last workgroup computes on whatever its LDS holds and stores nothing.
// The pixel permutation and dead-tap elimination of the 128-channel asm kernel are not here: padding MFMAs stay.
// Reference ops: neural_network.py:47-71,172-187 with eval-mode BatchNorm folded.
#include "../../include/xq_selfplay.h"
#include "xq_mfma.hpp"
#include "xq_tower_args.hpp"
#include <type_traits>

namespace {
using namespace xqm;

constexpr int PIX = 90, CH = 192, NB = 3;         // NB boards per workgroup, four waves each
constexpr int ROW = CH * 2;                       // one pixel's activations, bytes: 384 = 3 x 128
constexpr int ACT_BYTES = PIX * ROW;              // one board: 34,560
constexpr int WBUF_BYTES = CH * 128;              // one weight stage [192 cout][64 cin] bf16: 24,576
constexpr int ACT0 = 2 * WBUF_BYTES, ZROW = ACT0 + NB * ACT_BYTES, BIAS = ZROW + ROW;    // bias: [2][192] f32
constexpr int LDS_BYTES192 = BIAS + 2 * CH * 4;   // 154,752
constexpr int TILE = 16 * ROW;                    // a pixel tile's rows: the ds_read immediate of tile nt is nt * TILE
constexpr int SPL = 27;                           // weight stages per layer
constexpr int LAYER_BYTES = 9 * CH * ROW;         // one layer's weights [9][192][192] bf16
static_assert(LDS_BYTES192 == 154752 && LDS_BYTES192 <= 163840, "LDS plan");
static_assert(ACT0 % 128 == 0 && ACT_BYTES % 128 == 0 && ZROW % 128 == 0 && TILE % 128 == 0, "the low 7 bits of a row address are its slot");
static_assert(9 * CH * 32 <= ACT0 + ACT_BYTES - PIX * 32, "the input convolution's tap slices must end before board 0's planes");
static_assert(5 * TILE + 2 * 128 + 127 < 65536, "fragment immediates fit ds_read's 16-bit offset");

__global__ __launch_bounds__(768) void k_tower192(TowerArgs A)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wb_ = wave >> 2, qc = wave & 3;                         // board in workgroup, channel quarter
    int nrows = A.G;
    if (A.n_rows) { const int n = *A.n_rows; nrows = n < A.G ? n : A.G; }
    if ((int)blockIdx.x * NB >= nrows) return;     // compaction: no row for this workgroup (uniform, before any barrier / DMA)
    const int board = blockIdx.x * NB + wb_;
    const bool board_ok = board < nrows;
    const int act_off = ACT0 + wb_ * ACT_BYTES;
    const int r16 = lane & 15, q = lane >> 4;
    const int ch0 = qc * 48;                                          // row i of weight tile mt -> output channel ch0 + mt * 16 + i

    f32x4 acc[3][6];

    // ---------------------------------------------------------------- input conv (16 -> 192)
    const int pl_off = act_off + ACT_BYTES - PIX * 32;                // planes [90][16] bf16 in the tail of the board's region
    if (tid < ROW / 16) lds_st128(ZROW + tid * 16, make_uint4(0, 0, 0, 0));
    const int nlayers = 2 * A.nblocks, nstages = nlayers * SPL;
    if (wave == 1 && nstages > 0 && lane < CH / 4) dma16_abs(A.bias + CH + lane * 4, BIAS + CH * 4);   // bias[1] -> slot 1
#pragma unroll
    for (int j = 0; j < 5; j++) {                                     // w1: 54 pieces of 1 KB, unswizzled [9][192][16]
        const int piece = j * 12 + wave;
        if (piece < 54) dma16_abs(reinterpret_cast<const uint8_t *>(A.w1) + piece * 1024 + lane * 16, piece * 1024);
    }
    if (board_ok && qc < 3) {                                         // 180 chunks of 16 B: three waves of the board
        const int srow = A.row_src ? A.row_src[board] : board;      // (wave-uniform: a scalar load)
        const uint8_t *src = reinterpret_cast<const uint8_t *>(A.planes) + (size_t)srow * PIX * 32;
        const int idx = qc * 64 + lane;
        if (idx < PIX * 2) dma16_abs(src + idx * 16, pl_off + qc * 1024);
    }
#pragma unroll
    for (int mt = 0; mt < 3; mt++) {                                  // the accumulators start at this layer's bias
        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(A.bias + ch0 + mt * 16 + 4 * q);
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
            bf16x8 bf[6], af[3];
#pragma unroll
            for (int nt = 0; nt < 6; nt++) {
                const bool ok = tap_real && ((vm[nt / 3] >> ((nt % 3) * 9 + tp)) & 1u);
                const int sp = nt * 16 + r16 + off;
                bf[nt] = lds_ld128((ok ? pl_off + sp * 32 : ZROW + (sp & 7) * 32) + (q & 1) * 16);
            }
#pragma unroll
            for (int mt = 0; mt < 3; mt++)
                af[mt] = lds_ld128((tp * CH + ch0 + mt * 16 + r16) * 32 + (q & 1) * 16);
#pragma unroll
            for (int nt = 0; nt < 6; nt++)
#pragma unroll
                for (int mt = 0; mt < 3; mt++)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt], bf[nt], acc[mt][nt], 0, 0, 0);
        }
    }
    barrier_dma();                                                 // every wave is done with planes and tap slices
                                                                   // (its MFMAs consumed them: no LDS read is in flight)

    // ---------------------------------------------------------------- weight stream of the 192-channel layers
    // stage g = (layer, tap, K-slice g % 3): [192 cout][64 cin] -> buffer g & 1 as 192 rows of 128 B.  LDS row
    // rho = piece * 8 + (lane >> 3) holds the weights of channel rho: a scalar row offset per piece plus a lane part;
    // the 16-byte chunk at position c of row rho is source chunk c ^ (rho & 7)
    const rsrc_t wrsrc = make_rsrc(A.wt, nlayers * LAYER_BYTES);
    const int wsrc = (lane >> 3) * ROW + (((lane & 7) ^ (lane >> 3)) << 4);
    auto stage_piece = [&](int g, int buf, int j) {                   // j < 2 (past the end: the last stage again, into a dead buffer)
        const int gg = g < nstages ? g : nstages - 1;
        const int soff = (gg / 3) * (CH * ROW) + (gg % 3) * 128 + (wave * 2 + j) * 8 * ROW;
        dma16_buf_abs(wrsrc, wsrc, soff, buf * WBUF_BYTES + (wave * 2 + j) * 1024);
    };
    // A fragment (weight tile mt, K-step kk of a stage): abase ^ (kk << 6), + buf * WBUF_BYTES + mt * 2048
    const int abase = (ch0 + r16) * 128 + ((q ^ (r16 & 7)) << 4);
    auto load_a = [&](bf16x8 &af, int mt, int buf, int kk) {
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
    //   real pixel : act_off + sp * 384 + slot,  sp = r16 + tap offset (tile-independent: 16 | nt * 16)
    //   padding    : the zero row at the slot the lane's own row would have used
    const int Rrow = act_off + r16 * ROW, r5 = r16 << 4, q4 = q << 4;
    auto tap_addrs = [&](int (&as)[6], int tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1, off = dy * 9 + dx;
        // (an opaque copy of the row base per call keeps the tap's address arithmetic where it is written: hoisted
        // out of the block loop the 108 addresses would be spilled)
        int rrow = Rrow, r5o = r5;
        asm volatile("" : "+v"(rrow), "+v"(r5o));
        const int slot = ((r5o + off * 16) & 0x70) ^ q4;              // (q ^ (sp & 7)) << 4
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
    // (act_off, ZROW and TILE are multiples of 128: the low 7 bits of an address are its slot, the K-step's low bit an
    // XOR of 64 and its upper bits one of the row's three 128-byte groups)
    auto load_b = [&](bf16x8 &bf, int a, int nt, int ks) { bf = lds_ld128((a ^ ((ks & 1) << 6)) + (ks >> 1) * 128 + nt * TILE); };

    // epilogue of one layer: acc (bias [+ skip] already inside) -> bf16 -> ReLU -> LDS rows in place;
    // READ_X (first convolution of a block): the block input x is read back from those rows first and
    // the next layer's accumulators start at x + bias; otherwise they start at the next layer's bias
    auto epilogue = [&](auto read_x, int lb_next) {
        int ln;                                                       // lane id again, not CSE-able with the loop's
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
        const int r = ln & 15, qq = ln >> 4;
        const int rb = act_off + r * ROW;                             // pixel nt * 16 + r: + nt * TILE (p & 7 = r & 7 for every tile)
        const int rb5 = r < PIX - 80 ? rb + 5 * TILE : rb;            // the 6 slots past pixel 89 read pixel r and store nothing
        const int lbq = lb_next + (ch0 + qq * 4) * 4;                 // bias of channel ch0 + mt * 16 + qq * 4 ..
        // x + bias = S . X + bias: row i of the selector picks input channel i of the 16 that lane quarters 0 and 1 hold
        // (quarters 2 and 3 read them again and meet zeros), X = the tile's own 16 channels of the block input as 6
        // B fragments, bias as the C operand: one fp32 addition per element (exact products, the MFMA adder's rounding)
        bf16x8 sel;
        if constexpr (decltype(read_x)::value) {
#pragma unroll
            for (int j = 0; j < 8; j++) sel[j] = (qq == (r >> 3) && j == (r & 7)) ? (__bf16)1.0f : (__bf16)0.0f;
        }
#pragma unroll
        for (int mt = 0; mt < 3; mt++) {
            const f32x4 bn = lds_ldf4(lbq + mt * 64);
            bf16x8 xf[6];
            if constexpr (decltype(read_x)::value) {
                const int xo = (((qc * 6 + mt * 2 + (qq & 1)) ^ (r & 7)) << 4);
#pragma unroll
                for (int nt = 0; nt < 6; nt++) xf[nt] = lds_ld128((nt < 5 ? rb + nt * TILE : rb5) + xo);
            }
            const int so = (((qc * 6 + mt * 2 + (qq >> 1)) ^ (r & 7)) << 4) + (qq & 1) * 8;   // this lane's 4 channels of tile mt
#pragma unroll
            for (int nt = 0; nt < 6; nt++) {
                const f32x4 v = acc[mt][nt];
                const uint2 pk = make_uint2(relu_bf16x2(pack_bf16x2(v[0], v[1])), relu_bf16x2(pack_bf16x2(v[2], v[3])));
                if constexpr (decltype(read_x)::value)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sel, xf[nt], bn, 0, 0, 0);
                else
                    acc[mt][nt] = bn;
                if (nt < 5 || r < PIX - 80) lds_st64(rb + nt * TILE + so, pk);
            }
        }
    };
    using yes = std::integral_constant<bool, true>;
    using no = std::integral_constant<bool, false>;

    if (nstages > 0) {
#pragma unroll
        for (int j = 0; j < 2; j++) { stage_piece(0, 0, j); stage_piece(1, 1, j); }
    }
    epilogue(no{}, BIAS + CH * 4);                                  // conv1 output; tower layer 0 starts at bias[1]
    barrier_dma();

    // ---------------------------------------------------------------- residual tower
    bf16x8 fa[2][3], fb[6];                                          // weight fragments by K-step parity; activation fragments
    if (nstages > 0) {
#pragma unroll
        for (int mt = 0; mt < 3; mt++) load_a(fa[0][mt], mt, 0, 0);
    }
    // one layer; PAR = its parity in the block (a constant: stage sl of the layer sits in buffer (PAR + sl) & 1)
    auto conv_layer = [&](auto par, int layer) {
        constexpr int PAR = decltype(par)::value;
        if (wave == 1 && layer + 1 < nlayers && lane < CH / 4)      // bias of tower layer L + 1 (row L + 2) -> slot L & 1
            dma16_abs(A.bias + (size_t)(layer + 2) * CH + lane * 4, BIAS + PAR * CH * 4);
        const int g0 = layer * SPL;
        int as[6];
        tap_addrs(as, 0);
#pragma unroll
        for (int nt = 0; nt < 6; nt++) load_b(fb[nt], as[nt], nt, 0);
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            int asn[6];
#pragma unroll
            for (int ks = 0; ks < 6; ks++) {                        // 6 K-steps of 32 channels = 3 weight stages
                const int sl = tap * 3 + (ks >> 1);
                const int buf = (PAR + sl) & 1, kk = ks & 1, cur = ks & 1;
                const bool last = tap == 8 && ks == 5;                // last K-step of the layer: no activation prefetch
                if (ks == 5 && !last) tap_addrs(asn, tap + 1);
#pragma unroll
                for (int n = 0; n < 6; n++) {                        // pixel tile n: 3 MFMAs
#pragma unroll
                    for (int mt = 0; mt < 3; mt++)
                        acc[mt][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[cur][mt], fb[n], acc[mt][n], 0, 0, 0);
                    // this tile's activation fragment of the next K-step
                    if (!last) {
                        if (ks < 5) load_b(fb[n], as[n], n, ks + 1);
                        else load_b(fb[n], asn[n], n, 0);
                    }
                    // the next K-step's weight fragments (kk == 1: from the stage the barrier just published)
                    if (kk == 0 && n < 3) load_a(fa[cur ^ 1][n], n, buf, 1);
                    if (kk == 1 && n >= 1 && n < 4) load_a(fa[cur ^ 1][n - 1], n - 1, buf ^ 1, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (kk == 1 && n == 0) {
                        // stage barrier: the next stage has landed (every wave drains its own pieces first) and, this
                        // tile's MFMAs having consumed all 3 weight fragments of buffer buf, nobody reads it any more:
                        // the stage two ahead goes there
                        if (last) __builtin_amdgcn_s_waitcnt(0x0070);      // vmcnt(0) lgkmcnt(0): + all activation reads done
                        else __builtin_amdgcn_s_waitcnt(0x0F70);           // vmcnt(0)
                        __builtin_amdgcn_s_barrier();
                        __builtin_amdgcn_sched_barrier(0);
                        stage_piece(g0 + sl + 2, buf, 0);
                        stage_piece(g0 + sl + 2, buf, 1);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if (tap < 8) {
#pragma unroll
                for (int nt = 0; nt < 6; nt++) as[nt] = asn[nt];
            }
        }
        if constexpr (PAR) epilogue(no{}, BIAS + PAR * CH * 4);
        else epilogue(yes{}, BIAS + PAR * CH * 4);
        barrier_dma();
    };
    for (int blk = 0; blk < A.nblocks; blk++) {
        conv_layer(std::integral_constant<int, 0>{}, 2 * blk);
        conv_layer(std::integral_constant<int, 1>{}, 2 * blk + 1);
    }

    // ---------------------------------------------------------------- heads (1x1, 192 -> 32 + 8)
    {
        const uint8_t *src = reinterpret_cast<const uint8_t *>(A.wh);     // [64][384 B] -> buffer 0, chunk c of row rho at c ^ (rho & 7)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int q0 = (wave * 2 + j) * 64, idx = q0 + lane, row = idx / 24, cp = idx % 24;
            dma16_abs(src + row * ROW + ((cp ^ (row & 7)) * 16), q0 * 16);
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
    for (int ks = 0; ks < 6; ks++) {
        bf16x8 hb[6];
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const int p = nt * 16 + r16 < PIX ? nt * 16 + r16 : 0;
            hb[nt] = lds_ld128(act_off + p * ROW + (((ks * 4 + q) ^ (p & 7)) << 4));
        }
        const int row = qc * 16 + r16;
        const bf16x8 ha = lds_ld128(row * ROW + (((ks * 4 + q) ^ (row & 7)) << 4));
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

extern "C" int xq_tower192_nhwc_bf16(void *stream, const void *planes, const void *w1, const void *wt, const void *bias,
                                     const void *wh, const void *bh, void *policy_out, void *value_out, int n_boards,
                                     int n_blocks, const void *row_src_dev, const void *n_rows_dev)
{
    if (!planes || !w1 || !bias || !wh || !bh || !policy_out || !value_out || n_boards <= 0 || n_blocks < 0 ||
        (n_blocks > 0 && !wt) || n_blocks > 64)
        return XQ_E_INVALID;
    TowerArgs a{ (const uint16_t *)planes, (const uint16_t *)w1, (const uint16_t *)wt, (const float *)bias,
                 (const uint16_t *)wh, (const float *)bh, (uint16_t *)policy_out, (uint16_t *)value_out, n_boards, n_blocks,
                 nullptr, (const int32_t *)row_src_dev, (const int32_t *)n_rows_dev };
    if (int rc = tower_lds_opt_in<&k_tower192>(LDS_BYTES192)) return rc;
    hipLaunchKernelGGL(k_tower192, dim3((n_boards + NB - 1) / NB), dim3(768), LDS_BYTES192, reinterpret_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : XQ_E_HIP;
}
