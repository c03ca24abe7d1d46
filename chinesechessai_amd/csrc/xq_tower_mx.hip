// xq_tower_mx.hip — the whole convolutional trunk of a 128-channel policy/value network in ONE launch, with the
// 2 * nblocks tower convolutions on the block-scaled fp8 matrix pipe (OCP MXFP8: e4m3 elements, one E8M0 scale per 32).
//
//   planes [G][10][9][16] bf16  ->  conv3x3(16->128)+ReLU  ->  nblocks x { conv+ReLU, conv+skip+ReLU }
//                               ->  1x1 heads (policy 32, value 8)+ReLU  ->  P [G][90*32], V [G][90*8]
//
//   arithmetic   input convolution and heads: v_mfma_f32_16x16x32_bf16 on the bf16 tensors of the bf16 trunk.  Tower
//                convolutions: v_mfma_scale_f32_16x16x128_f8f6f4, both operands e4m3, fp32 accumulation, fp32 bias.
//                Every layer output is rounded to bf16 once (bias + convolution [+ skip, added in fp32], then ReLU);
//                the residual stream keeps that bf16 value; the next convolution's operand is derived from it per pixel
//                and block of 32 consecutive channels: m = block maximum, e = floor(log2 m) - 8 (+ 1 when m * 2^-e >
//                448: nothing saturates), scale byte = e + 127 clamped to 0..254 (127 for an all-zero block), elements
//                x * 2^(127 - byte) rounded to nearest-even e4m3 (neural_network.py: mx_quantize is the same rule).
//   work split   a wave = one board x all 128 output channels: weights on the MFMA rows, pixels on the columns, 6 pixel
//                tiles x 8 weight tiles = f32x4 acc[8][6], 192 accumulator registers, one wave per SIMD, 4 boards per
//                256-thread workgroup.  One 16x16x128 MFMA is one tap x all 128 input channels: lane (r, q) supplies 32 of
//                its row's / column's bytes (chunks q and q + 4, see lds_ld_frag) and the scale byte of channel block q.
//                A layer is 9 x 48 = 432 MFMAs per wave (the bf16 kernels: 1,728).
//   channel deal row i of weight tile mt is output channel (i >> 2) * 32 + mt * 4 + (i & 3).  The MFMA result gives lane
//                (r, q) rows 4q .. 4q + 3 of every weight tile for pixel column r: its 8 x 4 results of a pixel tile are
//                exactly channel block q of one pixel.  The epilogue is therefore all in-lane: block maximum, scale byte,
//                32 e4m3 bytes (two ds_write_b128), 64 bytes of the bf16 stream; the skip is the 64 bytes the same lane
//                wrote a block earlier.  The rows it wrote are what the next layer's lanes load as their B operand.
//   LDS          [weight ring 4 x 5,120][zero row 128, scale bytes 127: 128][stream 4 x 23,040][operand 4 x 11,520]
//                [scales 4 x 360] = 160,416 B of the CU's 163,840.  Rows are swizzled by pixel (chunk ^ (p & 7)):
//                the 16 pixels of a fragment load do not meet in one bank.  A wave owns its board: a layer's operand rows
//                are overwritten in place by that wave's own epilogue, no workgroup barrier is involved.
//   weights      one stream per workgroup for its 4 boards.  Stage s = (layer, tap, quarter): weight tiles 2 (s & 3) and
//                2 (s & 3) + 1 = 32 rows of 128 e4m3 bytes + 32 x 4 scale bytes, LDS-DMA into ring buffer s & 3: per wave
//                one 1 KB piece of the rows and one 256-byte piece (a dword per lane) that is the wave's own copy of the
//                scale bytes: the same two requests in every wave, so that s_waitcnt vmcnt is an exact count.  Step s:
//                vmcnt(4) lgkmcnt(0) + s_barrier publishes stage s + 1 and retires stage s (its fragments are in
//                registers), stage s + 4 is requested into the retired buffer, the fragments of
//                stage s + 1 are read, the 12 MFMAs of stage s run.  Past the last stage the requests repeat the last stage
//                (the counts stay exact); the heads' weights go to the operand rows, which are dead by then.
//   order        every output element is accumulated by one wave in one fixed order (bias [+ skip], taps 0..8) that
//                depends neither on G nor on the board's place in the launch or the workgroup: same planes -> same bits.
//                Boards at or beyond *n_rows: their workgroups return before any barrier or DMA; empty slots of the last
//                workgroup compute on whatever their LDS holds and store nothing.
//   compiler     scratch is 0 B with hipcc of ROCm 7.2.0 (AMD clang 22.0.0git): 192 accumulators leave little room, and three
//                things keep lane-derived addresses from being hoisted out of the layer loop and spilled - the lane id is
//                made again (v_mbcnt) for the tower, the epilogue and the heads, a tap's base goes through an opaque copy,
//                and the ring lies below 64 KB.  With another compiler check -Rpass-analysis=kernel-resource-usage again.
// Dead-tap elimination and the pixel permutation of the 128-channel asm kernel are not here: padding MFMAs stay.
// Reference ops: neural_network.py:47-71,172-187 with eval-mode BatchNorm folded.
#include "../../include/xq_selfplay.h"
#include "xq_mfma.hpp"
#include "xq_tower_args.hpp"
#include <type_traits>

namespace {
using namespace xqm;

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;

struct TowerMxArgs {
    TowerArgs t;               // t.wt: the e4m3 bytes [2*nblocks][9][128][128]
    const uint8_t *wscale;     // E8M0 scale bytes [2*nblocks][9][128][4]
};

constexpr int PIX = 90, CH = 128, NB = 4;            // NB boards per workgroup
constexpr int SROW = CH * 2, OROW = CH;              // a pixel's bf16 stream row / e4m3 operand row, bytes
// (the ring comes first: below 64 KB a fragment address is one lane register + a ds_read immediate)
constexpr int RING = 0, STAGE_W = 32 * OROW, STAGE = STAGE_W + NB * 256;   // 4,096 + a 256-byte copy of the 32 x 4 scale bytes per wave
constexpr int ZROW = RING + 4 * STAGE, ZSCL = ZROW + OROW;
constexpr int STREAM = ZSCL + 128, STREAM_B = PIX * SROW;              // 23,040 per board (every row base a multiple of 128:
                                                                       // chunk swizzles are XORs on the address)
constexpr int OPER = STREAM + NB * STREAM_B, OPER_B = PIX * OROW;      // 11,520 per board
constexpr int SCL = OPER + NB * OPER_B, SCL_B = PIX * 4;               // 360 per board
constexpr int LDS_BYTES_MX = SCL + NB * SCL_B;
constexpr int SPL = 36;                              // weight stages per layer
static_assert(STREAM == 20736 && LDS_BYTES_MX == 160416 && LDS_BYTES_MX <= 163840, "LDS plan");
static_assert(STREAM % 128 == 0 && OPER % 128 == 0 && STAGE % 128 == 0 && ZROW % 128 == 0 && OPER_B % 128 == 0 && STREAM_B % 128 == 0,
              "row bases are multiples of 128");
static_assert(9 * CH * 32 <= NB * STREAM_B, "the input convolution's tap slices lie in the stream region");
static_assert(48 * SROW <= NB * OPER_B, "the heads' weights fit the operand rows");

__device__ __forceinline__ uint32_t pkmax_u16(uint32_t a, uint32_t b)
{
    u16x2 x = *reinterpret_cast<u16x2 *>(&a), y = *reinterpret_cast<u16x2 *>(&b);
    x = __builtin_elementwise_max(x, y);
    return *reinterpret_cast<uint32_t *>(&x);
}
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wint-to-pointer-cast"
__device__ __forceinline__ int lds_ldu8(int off) { return *(const XQ_AS3 uint8_t *)(uint32_t)off; }
__device__ __forceinline__ void lds_stu8(int off, int v) { *(XQ_AS3 uint8_t *)(uint32_t)off = (uint8_t)v; }
__device__ __forceinline__ void dma4_buf_abs(rsrc_t rsrc, int voffset, int soffset, int lds_off)     // LDS: lds_off + lane * 4
{
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (XQ_AS3 void *)(uint32_t)lds_off, 4, voffset, soffset, 0, 0);
}
#pragma clang diagnostic pop

// The 32 operand bytes of lane (r, q) of a 16x16x128 MFMA, as the device showed them (a one-hot tower with cin in another
// block than cout came out unscaled): registers 0..3 are K 16q .. 16q + 15, registers 4..7 are K 64 + 16q .. 64 + 16q + 15,
// and the lane's scale byte belongs to K block q (K 32q .. 32q + 31), whose bytes lie in lanes (r, 2 (q & 1)) and
// (r, 2 (q & 1) + 1), registers 4 (q >> 1) ...  So a lane loads chunk q and chunk q + 4 of a 128-byte row - the first or
// second half of channel blocks q >> 1 and 2 + (q >> 1) - and still supplies the scale byte of ITS block q.  The
// epilogue is unchanged: a lane writes its own block's chunks 2q, 2q + 1 and scale byte.  addr: the row's chunk q (swizzled;
// row bases are multiples of 128, chunk q + 4 is addr ^ 64).
__device__ __forceinline__ i32x8 lds_ld_frag(int addr)
{
    const u32x4 lo = lds_ld128u(addr), hi = lds_ld128u(addr ^ 64);
    return i32x8{ (int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3] };
}

__global__ __launch_bounds__(256) void k_tower_mx(TowerMxArgs AM)
{
    const TowerArgs &A = AM.t;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // = board in workgroup
    int nrows = A.G;
    if (A.n_rows) { const int n = *A.n_rows; nrows = n < A.G ? n : A.G; }
    if ((int)blockIdx.x * NB >= nrows) return;      // compaction: no row for this workgroup (uniform, before any barrier / DMA)
    const int board = blockIdx.x * NB + wave;
    const bool board_ok = board < nrows;
    const int r16 = lane & 15, q = lane >> 4;
    const int stream_off = STREAM + wave * STREAM_B, oper_off = OPER + wave * OPER_B, scl_off = SCL + wave * SCL_B;
    // row i of weight tile mt -> output channel (see "channel deal" above)
    auto chan_row = [&](int mt, int i) { return (i >> 2) * 32 + mt * 4 + (i & 3); };

    f32x4 acc[8][6];

    // ---------------------------------------------------------------- input conv (16 -> 128), bf16
    const int nlayers = 2 * A.nblocks, nstages = nlayers * SPL;
    const int pl_off = oper_off;                                      // planes [90][16] bf16 in the board's own operand region
    if (tid < 8) lds_st128(ZROW + tid * 16, make_uint4(0, 0, 0, 0));
    if (tid == 8) lds_st128(ZSCL, make_uint4(0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu));
#pragma unroll
    for (int j = 0; j < 9; j++) {                                     // w1: 36 pieces of 1 KB, unswizzled [9][128][16]
        const int piece = j * 4 + wave;
        dma16_abs(reinterpret_cast<const uint8_t *>(A.w1) + piece * 1024 + lane * 16, STREAM + piece * 1024);
    }
    if (board_ok) {                                                   // 180 chunks of 16 B
        const int srow = A.row_src ? A.row_src[board] : board;      // (wave-uniform: a scalar load)
        const uint8_t *src = reinterpret_cast<const uint8_t *>(A.planes) + (size_t)srow * PIX * 32;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int idx = j * 64 + lane;
            if (idx < PIX * 2) dma16_abs(src + idx * 16, pl_off + j * 1024);
        }
    }
    // the weight stream of the tower: stage s -> ring buffer s & 3 (or the dump area past the end)
    const rsrc_t wrsrc = make_rsrc(A.wt, nlayers * 9 * CH * CH);
    const rsrc_t srsrc = make_rsrc(AM.wscale, nlayers * 9 * CH * 4);
    // piece `wave` of a stage: LDS rows wave * 8 + (lane >> 3), chunk lane & 7 <- source chunk (lane & 7) ^ (row & 7)
    const int wv_off = chan_row(wave >> 1, (wave & 1) * 8 + (lane >> 3)) * OROW + (((lane & 7) ^ ((lane >> 3) & 7)) << 4);
    // the 4 scale bytes of stage row lane & 31, one dword per lane: every wave fetches a copy of its own (twice: a request
    // of half a wave would be a branch in the step, and the compiler sinks the MFMAs of a step that has one)
    const int sv_off = chan_row((lane >> 4) & 1, lane & 15) * 4;
    auto stage_dma = [&](int s) {
        const int sc = s < nstages ? s : nstages - 1;                 // (past the end: the last stage again, the counts stay exact)
        const int dst = RING + (s & 3) * STAGE;
        dma16_buf_abs(wrsrc, wv_off, (sc >> 2) * (CH * CH) + (sc & 3) * (8 * OROW), dst + wave * 1024);
        dma4_buf_abs(srsrc, sv_off, (sc >> 2) * (CH * 4) + (sc & 3) * 32, dst + STAGE_W + wave * 256);
    };
    if (nstages > 0) {
#pragma unroll
        for (int s = 0; s < 4; s++) stage_dma(s);
    }
#pragma unroll
    for (int mt = 0; mt < 8; mt++) {                                  // the accumulators start at this layer's bias
        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(A.bias + chan_row(mt, 4 * q));
#pragma unroll
        for (int nt = 0; nt < 6; nt++) acc[mt][nt] = b4;
    }
    // tap validity of the 6 pixels of lane row r, 9 bits each
    auto tap_masks = [](int r, uint32_t (&vm)[2]) {
        vm[0] = vm[1] = 0;
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const int o = nt * 16 + r;
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
    };
    uint32_t vm[2];
    tap_masks(r16, vm);
    barrier_dma();
#pragma unroll
    for (int pair = 0; pair < 5; pair++) {                           // K-step = taps (2 pair, 2 pair + 1) x 16 planes
        const int tap = 2 * pair + (q >> 1);
        const bool tap_real = tap < 9;
        const int tp = tap_real ? tap : 8;
        const int off = (tp / 3 - 1) * 9 + (tp % 3 - 1);
        bf16x8 bf[6];
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const bool ok = tap_real && ((vm[nt / 3] >> ((nt % 3) * 9 + tp)) & 1u);
            const int sp = nt * 16 + r16 + off;
            bf[nt] = lds_ld128((ok ? pl_off + sp * 32 : ZROW) + (q & 1) * 16);
        }
#pragma unroll
        for (int mt = 0; mt < 8; mt++) {
            const bf16x8 af = lds_ld128(STREAM + (tp * CH + chan_row(mt, r16)) * 32 + (q & 1) * 16);
#pragma unroll
            for (int nt = 0; nt < 6; nt++)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf[nt], acc[mt][nt], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);                          // one K-step at a time (register pressure)
    }
    barrier_dma();                                                 // every wave is done with the tap slices (they lie
                                                                   // in the stream rows of boards 0 and 1)

    // epilogue of one layer: acc (bias [+ skip] already inside) -> bf16 -> ReLU -> this lane's channel block of 6 pixels:
    // scale byte, 32 e4m3 bytes and, with STREAM_OUT (input convolution, a block's second convolution), 64 bytes of the
    // bf16 stream.  Without it (a block's first convolution) the stream keeps the block input x and the next layer's
    // accumulators start at x + bias (fp32); otherwise they start at the next layer's bias.
    auto epilogue = [&](auto stream_out, const float *bias_next) {
        constexpr bool SO = decltype(stream_out)::value;
        int ln;                                                       // lane id again, not CSE-able with the loop's: the
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));   // addresses stay here
        const int r16 = ln & 15, q = ln >> 4;
        f32x4 bn[8];
#pragma unroll
        for (int mt = 0; mt < 8; mt++) {
            if (bias_next) bn[mt] = *reinterpret_cast<const f32x4 *>(bias_next + chan_row(mt, 4 * q));
            else bn[mt] = f32x4{ 0.f, 0.f, 0.f, 0.f };
        }
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            __builtin_amdgcn_sched_barrier(0);                      // one pixel tile at a time (register pressure)
            const int p = nt * 16 + r16;
            const bool real = nt < 5 || r16 < PIX - 80;
            const int pc = real ? p : 0;                              // (a clamped address for the lanes past pixel 89)
            const int sx = (pc & 7) << 4;
            uint32_t pk[16];
#pragma unroll
            for (int mt = 0; mt < 8; mt++) {
                const f32x4 v = acc[mt][nt];
                pk[2 * mt] = relu_bf16x2(pack_bf16x2(v[0], v[1]));
                pk[2 * mt + 1] = relu_bf16x2(pack_bf16x2(v[2], v[3]));
            }
            const int srow = stream_off + pc * SROW;
            if constexpr (SO) {
                if (real) {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        lds_st128(srow + ((((4 * q + k) << 4)) ^ sx), make_uint4(pk[4 * k], pk[4 * k + 1], pk[4 * k + 2], pk[4 * k + 3]));
                }
#pragma unroll
                for (int mt = 0; mt < 8; mt++) acc[mt][nt] = bn[mt];
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {                       // the block input x: the chunk this lane wrote a layer ago
                    const u32x4 x = lds_ld128u(srow + (((4 * q + k) << 4) ^ sx));
                    acc[2 * k][nt] = f32x4{ bn[2 * k][0] + bf16_lo(x[0]), bn[2 * k][1] + bf16_hi(x[0]),
                                            bn[2 * k][2] + bf16_lo(x[1]), bn[2 * k][3] + bf16_hi(x[1]) };
                    acc[2 * k + 1][nt] = f32x4{ bn[2 * k + 1][0] + bf16_lo(x[2]), bn[2 * k + 1][1] + bf16_hi(x[2]),
                                                bn[2 * k + 1][2] + bf16_lo(x[3]), bn[2 * k + 1][3] + bf16_hi(x[3]) };
                }
            }
            // block maximum (the values are >= +0 after the ReLU: their bf16 patterns order like unsigned integers)
            uint32_t m2 = pk[0];
#pragma unroll
            for (int k = 1; k < 16; k++) m2 = pkmax_u16(m2, pk[k]);
            const uint32_t mb = (m2 & 0xffffu) > (m2 >> 16) ? (m2 & 0xffffu) : (m2 >> 16);
            const int ex = (int)(mb >> 7);                            // biased exponent of m
            int sb = ex >= 8 ? ex - 8 + ((mb & 0x7fu) > 0x60u ? 1 : 0) : 0;        // mantissa above 1.75: m * 2^-e > 448
            if (mb == 0) sb = 127;
            const float mult = __uint_as_float((uint32_t)(254 - sb) << 23);       // 2^(127 - sb)
            uint32_t w8[8];
#pragma unroll
            for (int mt = 0; mt < 8; mt++) {
                int w = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_lo(pk[2 * mt]) * mult, bf16_hi(pk[2 * mt]) * mult, 0, false);
                w = __builtin_amdgcn_cvt_pk_fp8_f32(bf16_lo(pk[2 * mt + 1]) * mult, bf16_hi(pk[2 * mt + 1]) * mult, w, true);
                w8[mt] = (uint32_t)w;
            }
            if (real) {
                const int orow = oper_off + pc * OROW;
                lds_st128(orow + (((2 * q) << 4) ^ sx), make_uint4(w8[0], w8[1], w8[2], w8[3]));
                lds_st128(orow + (((2 * q + 1) << 4) ^ sx), make_uint4(w8[4], w8[5], w8[6], w8[7]));
                lds_stu8(scl_off + pc * 4 + q, sb);
            }
        }
    };
    using yes = std::integral_constant<bool, true>;
    using no = std::integral_constant<bool, false>;

    epilogue(yes{}, nlayers > 0 ? A.bias + CH : nullptr);           // conv1 output; tower layer 0 starts at bias[1]

    // ---------------------------------------------------------------- residual tower, MXFP8
    // B operand of (pixel tile nt, tap): the e4m3 row and the scale byte of the neighbour pixel, or the zero row with
    // scale byte 127 where the tap reads padding
    int lt;                                                         // (lane id again: the tower's lane values are made here)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lt));
    [&](const int r16, const int q) {
    uint32_t vm[2];
    tap_masks(r16, vm);
    int a0, a1;
    uint32_t v0, v1;
    auto tap_base = [&](int tap) {
        const int off = (tap / 3 - 1) * 9 + (tap % 3 - 1);
        // (opaque copies per call keep the tap's address arithmetic where it is written: hoisted out of the layer loop
        // the 108 addresses would be spilled)
        int r = r16;
        v0 = vm[0], v1 = vm[1];
        asm volatile("" : "+v"(r), "+v"(v0), "+v"(v1));
        const int sp0 = r + off;                                      // (16 | nt * 16: the swizzle is tile-independent)
        a0 = oper_off + sp0 * OROW + ((q << 4) ^ ((sp0 & 7) << 4)), a1 = scl_off + sp0 * 4 + q;
    };
    auto load_b1 = [&](i32x8 &fb, int &sbv, int tap, int nt) {       // after tap_base(tap)
        const bool ok = ((nt < 3 ? v0 : v1) >> ((nt % 3) * 9 + tap)) & 1u;
        fb = lds_ld_frag(ok ? a0 + nt * 16 * OROW : ZROW + q * 16);
        sbv = lds_ldu8(ok ? a1 + nt * 64 : ZSCL + q);
    };
    // A operand: weight tile j (0, 1) of ring buffer buf, row j * 16 + r16, chunks 2q, 2q + 1 (swizzled by the row)
    auto load_a = [&](i32x8 (&fa)[2], int (&sav)[2], int buf) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int row = j * 16 + r16;
            fa[j] = lds_ld_frag(RING + buf * STAGE + row * OROW + ((q << 4) ^ ((row & 7) << 4)));
            sav[j] = lds_ldu8(RING + buf * STAGE + STAGE_W + wave * 256 + row * 4 + q);
        }
    };
    if (nstages > 0) {
        i32x8 fa[2][2], fb[6];
        int sa[2][2], sbv[6];
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0x0F76);                          // vmcnt(6): stage 0 has landed (1, 2, 3 are behind it)
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        load_a(fa[0], sa[0], 0);
        for (int layer = 0; layer < nlayers; layer++) {
            tap_base(0);
#pragma unroll
            for (int nt = 0; nt < 6; nt++) load_b1(fb[nt], sbv[nt], 0, nt);
#pragma unroll
            for (int tap = 0; tap < 9; tap++) {
#pragma unroll
                for (int qt = 0; qt < 4; qt++) {
                    const int s = layer * SPL + tap * 4 + qt, cur = qt & 1;
                    // step barrier: stage s + 1 has landed (every wave drains its own pieces: s + 2, s + 3 are behind
                    // them) and every wave holds its fragments of stage s in registers: buffer s & 3 is free
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_waitcnt(0x0074);              // vmcnt(4) lgkmcnt(0)
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    stage_dma(s + 4);
                    load_a(fa[cur ^ 1], sa[cur ^ 1], (qt + 1) & 3);
                    // the tap's last step fetches the next tap's B operands, each tile behind its last use (one copy of
                    // the 48 operand registers: two do not fit beside 192 accumulators without scratch)
                    const bool next_b = qt == 3 && tap < 8;
                    if (next_b) tap_base(tap + 1);
#pragma unroll
                    for (int nt = 0; nt < 6; nt++) {
#pragma unroll
                        for (int j = 0; j < 2; j++)
                            acc[2 * qt + j][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                                fa[cur][j], fb[nt], acc[2 * qt + j][nt], 0, 0, 0, sa[cur][j], 0, sbv[nt]);
                        if (next_b) load_b1(fb[nt], sbv[nt], tap + 1, nt);
                    }
                }
            }
            // (fa[0] now holds the first stage of the next layer: 36 steps, an even number)
            const float *bias_next = layer + 1 < nlayers ? A.bias + (size_t)(layer + 2) * CH : nullptr;
            if (layer & 1) epilogue(yes{}, bias_next);
            else epilogue(no{}, bias_next);
        }
    }
    }(lt & 15, lt >> 4);

    // ---------------------------------------------------------------- heads (1x1, 128 -> 32 + 8), bf16
    barrier_dma();                                                 // every wave is done with its operand rows
    int lh;                                                         // (lane id again: nothing of the heads lives through the tower)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lh));
    [&](const int lane, const int r16, const int q) {
    {
        const uint8_t *src = reinterpret_cast<const uint8_t *>(A.wh);     // rows 0..47 [256 B] -> the operand region, chunk ^ (row & 7)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int q0 = (wave * 3 + j) * 64, idx = q0 + lane, row = idx >> 4, cp = idx & 15;
            dma16_abs(src + row * SROW + ((cp ^ (row & 7)) << 4), OPER + q0 * 16);
        }
    }
    f32x4 hacc[3][6];
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
        for (int nt = 0; nt < 6; nt++) hacc[t][nt] = f32x4{ 0.f, 0.f, 0.f, 0.f };
    barrier_dma();
    if (!board_ok) return;                                           // (no barrier follows)
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {                                 // K-step ks: channels 32 ks + 8 q ..
        bf16x8 hb[6];
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const int p = nt * 16 + r16 < PIX ? nt * 16 + r16 : 0;
            hb[nt] = lds_ld128(stream_off + p * SROW + (((4 * ks + q) ^ (p & 7)) << 4));
        }
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const int row = t * 16 + r16;
            const bf16x8 ha = lds_ld128(OPER + row * SROW + (((4 * ks + q) ^ (row & 7)) << 4));
#pragma unroll
            for (int nt = 0; nt < 6; nt++)
                hacc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha, hb[nt], hacc[t][nt], 0, 0, 0);
        }
    }
    uint8_t *Pb = reinterpret_cast<uint8_t *>(A.P) + (size_t)board * PIX * 64;
    uint8_t *Vb = reinterpret_cast<uint8_t *>(A.V) + (size_t)board * PIX * 16;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        if (t == 2 && q >= 2) continue;                              // value head: channels 32..39 only
        const int c0 = t * 16 + 4 * q;                               // head channel of element 0
        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(A.bh + c0);
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const int p = nt * 16 + r16;
            if (p < PIX) {
                const f32x4 h = hacc[t][nt];
                const uint2 pk = make_uint2(relu_bf16x2(pack_bf16x2(h[0] + b4[0], h[1] + b4[1])),
                                            relu_bf16x2(pack_bf16x2(h[2] + b4[2], h[3] + b4[3])));
                if (t < 2) *reinterpret_cast<uint2 *>(Pb + p * 64 + c0 * 2) = pk;
                else *reinterpret_cast<uint2 *>(Vb + p * 16 + (c0 - 32) * 2) = pk;
            }
        }
    }
    }(lh, lh & 15, lh >> 4);
}

}  // namespace

extern "C" int xq_tower_mxfp8_nhwc(void *stream, const void *planes, const void *w1, const void *wq, const void *wscale,
                                   const void *bias, const void *wh, const void *bh, void *policy_out, void *value_out,
                                   int n_boards, int n_blocks, const void *row_src_dev, const void *n_rows_dev)
{
    if (!planes || !w1 || !bias || !wh || !bh || !policy_out || !value_out || n_boards <= 0 || n_blocks < 0 ||
        (n_blocks > 0 && (!wq || !wscale)) || n_blocks > 64)
        return XQ_E_INVALID;
    TowerMxArgs a{ { (const uint16_t *)planes, (const uint16_t *)w1, (const uint16_t *)wq, (const float *)bias,
                     (const uint16_t *)wh, (const float *)bh, (uint16_t *)policy_out, (uint16_t *)value_out, n_boards, n_blocks,
                     nullptr, (const int32_t *)row_src_dev, (const int32_t *)n_rows_dev },
                   (const uint8_t *)wscale };
    if (int rc = tower_lds_opt_in<&k_tower_mx>(LDS_BYTES_MX)) return rc;
    hipLaunchKernelGGL(k_tower_mx, dim3((n_boards + NB - 1) / NB), dim3(256), LDS_BYTES_MX, reinterpret_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : XQ_E_HIP;
}
