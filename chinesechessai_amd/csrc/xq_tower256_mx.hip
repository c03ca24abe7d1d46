// xq_tower256_mx.hip — the whole convolutional trunk of a 256-channel policy/value network in ONE launch, with the
// 2 * nblocks tower convolutions on the block-scaled fp8 matrix pipe (OCP MXFP8: e4m3 elements, one E8M0 scale per 32).
//
//   planes [G][10][9][16] bf16  ->  conv3x3(16->256)+ReLU  ->  nblocks x { conv+ReLU, conv+skip+ReLU }
//                               ->  1x1 heads (policy 32, value 8)+ReLU  ->  P [G][90*32], V [G][90*8]
//
//   arithmetic   the rule of k_tower_mx (xq_tower_mx.hip): input convolution and heads v_mfma_f32_16x16x32_bf16 on the bf16
//                tensors of the bf16 trunk; tower convolutions v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 x e4m3, fp32
//                accumulation, fp32 bias as the accumulator start.  Every layer output is rounded to bf16 once (bias +
//                convolution [+ skip, added in fp32], then ReLU); the residual stream keeps that bf16 value; the next
//                operand is that value quantised per pixel and block of 32 consecutive channels by mx_quantize's rule
//                (neural_network.py): scale byte = e + 127 clamped to 0..254, 127 for an all-zero block, the "+ 1" so that
//                nothing exceeds 448.
//   work split   a wave = one board x a 128-channel HALF h of the output channels: weights on the MFMA rows, pixels on the
//                columns, 6 pixel tiles x 8 weight tiles = f32x4 acc[8][6], 192 accumulator registers, one wave per SIMD,
//                2 boards per 256-thread workgroup (wave = 2 * board + h), one workgroup per CU.  One 16x16x128 MFMA is one
//                tap x one K-half kh of 128 input channels: per wave and layer 9 x 2 x 48 = 864 MFMAs, 1,728 per board
//                (k_tower256: 6,912).
//   channel deal row i of weight tile mt of half h is output channel h * 128 + (i >> 2) * 32 + mt * 4 + (i & 3).  Lane (r, q)
//                gets rows 4q .. 4q + 3 of every weight tile for pixel column r: its 8 x 4 results of a pixel are exactly
//                channel block 4h + q.  The epilogue is all in-lane as in k_tower_mx: block maximum, scale byte, 32 e4m3
//                bytes, 64 bytes of the bf16 stream; the skip is the 64 bytes the same lane wrote a block earlier.
//   operands     a pixel's operand row is 256 bytes = two K-halves of 128; the 8 chunks of each half are swizzled by
//                pixel & 7.  For K-half kh lane (r, q) loads chunks q and q + 4 of that half (registers 0..3: K 16q ..,
//                registers 4..7: K 64 + 16q ..) and supplies the scale byte of block 4 kh + q (the layout the
//                device showed).  A wave's epilogue writes K-half h of its board's rows and scale bytes 4h .. 4h + 3.
//   two waves, one board   the sibling wave reads the whole operand row, so a store of layer L + 1's operand must follow
//                every read of layer L by BOTH waves.  The last operand reads of a layer (tap 8, K-half 1) are issued in
//                step (8, 0, 7); each of the 8 steps behind it begins with s_waitcnt lgkmcnt(0) + s_barrier, so every wave
//                has them in registers long before any wave reaches the epilogue.  Behind the epilogue a second barrier
//                (lgkmcnt(0) + s_barrier, layer_barrier) publishes both halves before the first reads of layer L + 1.
//                The stream rows a wave re-reads for the skip are its own 128 channels: no barrier.
//   LDS          [weight ring 4 x 5,120][zero row 256, scale bytes 127: 128][stream 2 x 46,080][operand 2 x 23,040]
//                [scales 2 x 720] = 160,544 B of the CU's 163,840.  The ring lies below 64 KB.
//   weights      one stream per workgroup for both boards.  Stage s = (layer, tap, K-half, weight tile mt): the 16 rows of
//                tile mt of both halves = 32 rows of 128 e4m3 bytes = 4,096 B + per wave a 256-byte piece (a dword per
//                lane) with the 16 x 4 scale bytes of its own half's rows: stage size 5,120 B, ring depth 4, the same two
//                LDS-DMA requests in every wave and step, so that s_waitcnt vmcnt is an exact count.  144 stages per
//                layer (a multiple of 4: the buffer of a stage is a constant of the unrolled loop).  Step s:
//                s_waitcnt vmcnt(4) lgkmcnt(0) + s_barrier publishes stage s + 1 (the 4 requests still out are stages
//                s + 2, s + 3) and retires stage s (its fragments are in registers); stage s + 4 is requested into the
//                retired buffer; the fragments of stage s + 1 are read; the 6 MFMAs of stage s run.  A request has 3 steps
//                = 18 MFMAs = 576 MFMA cycles of cover (k_tower_mx: 3 x 12 MFMAs).  Before the first step:
//                s_waitcnt vmcnt(6) lgkmcnt(0) + s_barrier (stage 0 landed, the input convolution's epilogue published).
//                Past the last stage the requests repeat the last stage.
//   staging      w1 [9][256][16] (73,728 B) lies over both boards' stream rows during the input convolution, the planes in
//                each board's operand rows; the heads' weights (48 rows of 512 B) go over the operand rows after the tower.
//   order        every output element is accumulated by one wave in one fixed order (bias [+ skip], taps 0..8, K-halves
//                0..1) that depends neither on G nor on the board's place in the launch or the workgroup: same planes ->
//                same bits.  Boards at or beyond *n_rows: their workgroups return before any barrier or DMA; the empty
//                second slot of the last workgroup computes on whatever its LDS holds and stores nothing.
//   compiler     as k_tower_mx: the lane id is made again (v_mbcnt) for the tower, the epilogue and the heads, a tap's
//                base goes through an opaque copy, the ring lies below 64 KB.  Check scratch with
//                -Rpass-analysis=kernel-resource-usage after a compiler change (DESIGN §5 has the figures).
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

struct Tower256MxArgs {
    TowerArgs t;               // t.wt: the e4m3 bytes [2*nblocks][9][256][256]
    const uint8_t *wscale;     // E8M0 scale bytes [2*nblocks][9][256][8]
};

constexpr int PIX = 90, CH = 256, NB = 2;            // NB boards per workgroup
constexpr int SROW = CH * 2, OROW = CH, WROW = 128;  // a pixel's bf16 stream row / e4m3 operand row / a ring row (one K-half), bytes
constexpr int RING = 0, STAGE_W = 32 * WROW, STAGE = STAGE_W + 4 * 256;    // 4,096 + a 256-byte scale piece per wave
constexpr int ZROW = RING + 4 * STAGE, ZSCL = ZROW + OROW;
constexpr int STREAM = ZSCL + 128, STREAM_B = PIX * SROW;              // 46,080 per board (every row base a multiple of 128:
                                                                       // chunk swizzles are XORs on the address)
constexpr int OPER = STREAM + NB * STREAM_B, OPER_B = PIX * OROW;      // 23,040 per board
constexpr int SCL = OPER + NB * OPER_B, SCL_B = PIX * 8;               // 720 per board
constexpr int LDS_BYTES_MX256 = SCL + NB * SCL_B;
constexpr int SPL = 144;                             // weight stages per layer
static_assert(STREAM == 20864 && LDS_BYTES_MX256 == 160544 && LDS_BYTES_MX256 <= 163840 && ZSCL + 128 <= 65536, "LDS plan");
static_assert(STREAM % 128 == 0 && OPER % 128 == 0 && STAGE % 128 == 0 && ZROW % 128 == 0 && OPER_B % 128 == 0 && STREAM_B % 128 == 0,
              "row bases are multiples of 128");
static_assert(9 * CH * 32 <= NB * STREAM_B, "the input convolution's tap slices lie in the stream region");
static_assert(48 * SROW <= NB * OPER_B && PIX * 32 <= OPER_B, "the heads' weights and a board's planes fit the operand rows");
static_assert(SPL % 4 == 0, "a stage's ring buffer is a constant of the unrolled layer");

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

// The 32 operand bytes of lane (r, q) of a 16x16x128 MFMA (xq_tower_mx.hip has the derivation): chunk q and chunk q + 4 of
// a 128-byte K-half.  addr: the half's chunk q (swizzled; half bases are multiples of 128, chunk q + 4 is addr ^ 64).
__device__ __forceinline__ i32x8 lds_ld_frag(int addr)
{
    const u32x4 lo = lds_ld128u(addr), hi = lds_ld128u(addr ^ 64);
    return i32x8{ (int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3] };
}

// every LDS access of this wave is complete, then every wave's: publishes a layer's epilogue stores to the sibling wave
// (vmcnt is left alone: the weight ring's requests stay in flight)
__device__ __forceinline__ void layer_barrier()
{
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);                                // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

__global__ __launch_bounds__(256) void k_tower256_mx(Tower256MxArgs AM)
{
    const TowerArgs &A = AM.t;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wb = wave >> 1, h = wave & 1;                           // board in workgroup, channel half
    int nrows = A.G;
    if (A.n_rows) { const int n = *A.n_rows; nrows = n < A.G ? n : A.G; }
    if ((int)blockIdx.x * NB >= nrows) return;      // compaction: no row for this workgroup (uniform, before any barrier / DMA)
    const int board = blockIdx.x * NB + wb;
    const bool board_ok = board < nrows;
    const int r16 = lane & 15, q = lane >> 4;
    const int stream_off = STREAM + wb * STREAM_B, oper_off = OPER + wb * OPER_B, scl_off = SCL + wb * SCL_B;
    // row i of weight tile mt of this wave's half -> output channel (see "channel deal" above)
    auto chan_row = [&](int mt, int i) { return h * 128 + (i >> 2) * 32 + mt * 4 + (i & 3); };

    f32x4 acc[8][6];

    // ---------------------------------------------------------------- input conv (16 -> 256), bf16
    const int nlayers = 2 * A.nblocks, nstages = nlayers * SPL;
    const int pl_off = oper_off;                                      // planes [90][16] bf16 in the board's own operand region
    if (tid < 16) lds_st128(ZROW + tid * 16, make_uint4(0, 0, 0, 0));
    if (tid >= 16 && tid < 24) lds_st128(ZSCL + (tid - 16) * 16, make_uint4(0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu, 0x7f7f7f7fu));
#pragma unroll
    for (int j = 0; j < 18; j++) {                                    // w1: 72 pieces of 1 KB, unswizzled [9][256][16]
        const int piece = j * 4 + wave;
        dma16_abs(reinterpret_cast<const uint8_t *>(A.w1) + piece * 1024 + lane * 16, STREAM + piece * 1024);
    }
    if (board_ok) {                                                   // 180 chunks of 16 B: pieces h and h + 2 of the board's three
        const int srow = A.row_src ? A.row_src[board] : board;      // (wave-uniform: a scalar load)
        const uint8_t *src = reinterpret_cast<const uint8_t *>(A.planes) + (size_t)srow * PIX * 32;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int idx = (2 * j + h) * 64 + lane;
            if (idx < PIX * 2) dma16_abs(src + idx * 16, pl_off + (2 * j + h) * 1024);
        }
    }
    // the weight stream of the tower: stage s -> ring buffer s & 3
    const rsrc_t wrsrc = make_rsrc(A.wt, nlayers * 9 * CH * CH);
    const rsrc_t srsrc = make_rsrc(AM.wscale, nlayers * 9 * CH * 8);
    // piece `wave` of a stage: ring rows wave * 8 + (lane >> 3) = rows (wave & 1) * 8 .. of half wave >> 1 (NOT this wave's
    // own half: the four pieces are the stage), chunk lane & 7 <- source chunk (lane & 7) ^ (row & 7) of the K-half
    const int wrow = (wave & 1) * 8 + (lane >> 3);
    const int wv_off = ((wave >> 1) * 128 + (wrow >> 2) * 32 + (wrow & 3)) * OROW + (((lane & 7) ^ ((lane >> 3) & 7)) << 4);
    // the 4 scale bytes (blocks 4 kh .. 4 kh + 3) of row lane & 15 of this wave's own half, one dword per lane: every wave
    // fetches its own copy, four times over (a request of a quarter wave would be a branch in the step)
    const int sv_off = chan_row(0, lane & 15) * 8;
    auto stage_dma = [&](int s) {
        const int sc = s < nstages ? s : nstages - 1;                 // (past the end: the last stage again, the counts stay exact)
        const int dst = RING + (s & 3) * STAGE;
        const int lt = sc >> 4, kh = (sc >> 3) & 1, mt = sc & 7;      // (layer * 9 + tap, K-half, weight tile)
        dma16_buf_abs(wrsrc, wv_off, lt * (CH * CH) + kh * 128 + mt * (4 * OROW), dst + wave * 1024);
        dma4_buf_abs(srsrc, sv_off, lt * (CH * 8) + kh * 4 + mt * 32, dst + STAGE_W + wave * 256);
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
    barrier_dma();                                                 // every wave is done with the tap slices (they lie in
                                                                   // the stream rows) and with its board's planes (the
                                                                   // sibling's epilogue overwrites them)

    // epilogue of one layer: acc (bias [+ skip] already inside) -> bf16 -> ReLU -> this lane's channel block 4h + q of 6
    // pixels: scale byte, 32 e4m3 bytes and, with STREAM_OUT (input convolution, a block's second convolution), 64 bytes of
    // the bf16 stream.  Without it (a block's first convolution) the stream keeps the block input x and the next layer's
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
            const int srow = stream_off + pc * SROW, c0 = h * 16 + 4 * q;         // chunks 4 (4h + q) .. + 3 of the stream row
            if constexpr (SO) {
                if (real) {
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        lds_st128(srow + (((c0 + k) << 4) ^ sx), make_uint4(pk[4 * k], pk[4 * k + 1], pk[4 * k + 2], pk[4 * k + 3]));
                }
#pragma unroll
                for (int mt = 0; mt < 8; mt++) acc[mt][nt] = bn[mt];
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {                       // the block input x: the chunk this lane wrote a layer ago
                    const u32x4 x = lds_ld128u(srow + (((c0 + k) << 4) ^ sx));
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
                const int orow = oper_off + pc * OROW + h * 128;      // K-half h of the operand row
                lds_st128(orow + (((2 * q) << 4) ^ sx), make_uint4(w8[0], w8[1], w8[2], w8[3]));
                lds_st128(orow + (((2 * q + 1) << 4) ^ sx), make_uint4(w8[4], w8[5], w8[6], w8[7]));
                lds_stu8(scl_off + pc * 8 + 4 * h + q, sb);
            }
        }
    };
    using yes = std::integral_constant<bool, true>;
    using no = std::integral_constant<bool, false>;

    epilogue(yes{}, nlayers > 0 ? A.bias + CH : nullptr);           // conv1 output; tower layer 0 starts at bias[1]

    // ---------------------------------------------------------------- residual tower, MXFP8
    // B operand of (pixel tile nt, tap, K-half): the e4m3 half row and the scale byte of the neighbour pixel, or the zero
    // row with scale byte 127 where the tap reads padding
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
        // the addresses would be spilled)
        int r = r16, qq = q;
        v0 = vm[0], v1 = vm[1];
        asm volatile("" : "+v"(r), "+v"(qq), "+v"(v0), "+v"(v1));
        const int sp0 = r + off;                                      // (16 | nt * 16: the swizzle is tile-independent)
        a0 = oper_off + sp0 * OROW + ((qq << 4) ^ ((sp0 & 7) << 4)), a1 = scl_off + sp0 * 8 + qq;
    };
    auto load_b1 = [&](i32x8 &fb, int &sbv, int tap, int kh, int nt) {       // after tap_base(tap)
        const bool ok = ((nt < 3 ? v0 : v1) >> ((nt % 3) * 9 + tap)) & 1u;
        fb = lds_ld_frag(ok ? a0 + nt * 16 * OROW + kh * 128 : ZROW + q * 16);
        sbv = lds_ldu8(ok ? a1 + nt * 128 + kh * 4 : ZSCL + q);
    };
    // A operand: this half's weight tile of ring buffer buf, row h * 16 + r16, chunks q, q + 4 (swizzled by the row)
    const int fa_lo = RING + (h * 16 + r16) * WROW + ((q << 4) ^ ((r16 & 7) << 4)), fa_hi = fa_lo ^ 64;
    const int sa_ad = RING + STAGE_W + wave * 256 + r16 * 4 + q;
    auto load_a = [&](i32x8 &fa, int &sav, int buf) {
        // (one address pair and one scale address for all four buffers: buf * STAGE is the ds_read immediate)
        const u32x4 lo = lds_ld128u(fa_lo + buf * STAGE), hi = lds_ld128u(fa_hi + buf * STAGE);
        fa = i32x8{ (int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3] };
        sav = lds_ldu8(sa_ad + buf * STAGE);
    };
    if (nstages > 0) {
        i32x8 fa[2], fb[6];
        int sa[2], sbv[6];
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0x0076);                          // vmcnt(6) lgkmcnt(0): stage 0 has landed (1, 2, 3 are
        __builtin_amdgcn_s_barrier();                                // behind it), the input convolution's epilogue is published
        __builtin_amdgcn_sched_barrier(0);
        load_a(fa[0], sa[0], 0);
        for (int layer = 0; layer < nlayers; layer++) {
            tap_base(0);
#pragma unroll
            for (int nt = 0; nt < 6; nt++) load_b1(fb[nt], sbv[nt], 0, 0, nt);
#pragma unroll
            for (int tk = 0; tk < 18; tk++) {                        // (tap, K-half)
#pragma unroll
                for (int mt = 0; mt < 8; mt++) {
                    const int cur = mt & 1;
                    // step barrier: stage s + 1 has landed (every wave drains its own pieces: s + 2, s + 3 are behind
                    // them) and every wave holds its fragments of stage s in registers: buffer s & 3 is free
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_waitcnt(0x0074);              // vmcnt(4) lgkmcnt(0)
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    stage_dma(layer * SPL + tk * 8 + mt + 4);
                    load_a(fa[cur ^ 1], sa[cur ^ 1], (mt + 1) & 3);
                    // the last step of a (tap, K-half) fetches the next one's B operands, each tile behind its last use
                    // (one copy of the 48 operand registers)
                    const bool next_b = mt == 7 && tk < 17;
                    if (next_b) tap_base((tk + 1) >> 1);
#pragma unroll
                    for (int nt = 0; nt < 6; nt++) {
                        acc[mt][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                            fa[cur], fb[nt], acc[mt][nt], 0, 0, 0, sa[cur], 0, sbv[nt]);
                        if (next_b) load_b1(fb[nt], sbv[nt], (tk + 1) >> 1, (tk + 1) & 1, nt);
                    }
                }
            }
            // (fa[0] now holds the first stage of the next layer: 144 steps, an even number.  Every operand read of this
            // layer was complete at the barrier of step (8, 1, 0), in both waves of the board)
            const float *bias_next = layer + 1 < nlayers ? A.bias + (size_t)(layer + 2) * CH : nullptr;
            if (layer & 1) epilogue(yes{}, bias_next);
            else epilogue(no{}, bias_next);
            layer_barrier();                                         // both halves of the new operand rows are there
        }
    }
    }(lt & 15, lt >> 4);

    // ---------------------------------------------------------------- heads (1x1, 256 -> 32 + 8), bf16
    barrier_dma();                                                 // every wave is done with the operand rows; the
                                                                   // stream rows of both halves are published
    int lh;                                                         // (lane id again: nothing of the heads lives through the tower)
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lh));
    [&](const int lane, const int r16, const int q) {
    {
        const uint8_t *src = reinterpret_cast<const uint8_t *>(A.wh);     // rows 0..47 [512 B] -> the operand region, chunk ^ (row & 7)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const int q0 = (wave * 6 + j) * 64, idx = q0 + lane, row = idx >> 5, cp = idx & 31;
            dma16_abs(src + row * SROW + ((cp ^ (row & 7)) << 4), OPER + q0 * 16);
        }
    }
    // wave h = 0 of a board: head rows 0..31 (policy), wave h = 1: rows 32..47 (value channels 32..39 and 8 zero rows)
    f32x4 hacc[2][6];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int nt = 0; nt < 6; nt++) hacc[t][nt] = f32x4{ 0.f, 0.f, 0.f, 0.f };
    barrier_dma();
    if (!board_ok) return;                                           // (no barrier follows)
    const int nth = h ? 1 : 2;
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {                                 // K-step ks: channels 32 ks + 8 q ..
        bf16x8 hb[6];
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const int p = nt * 16 + r16 < PIX ? nt * 16 + r16 : 0;
            hb[nt] = lds_ld128(stream_off + p * SROW + (((4 * ks + q) ^ (p & 7)) << 4));
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {
            if (t >= nth) continue;                                  // (wave-uniform)
            const int row = (2 * h + t) * 16 + r16;
            const bf16x8 ha = lds_ld128(OPER + row * SROW + (((4 * ks + q) ^ (row & 7)) << 4));
#pragma unroll
            for (int nt = 0; nt < 6; nt++)
                hacc[t][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ha, hb[nt], hacc[t][nt], 0, 0, 0);
        }
    }
    uint8_t *Pb = reinterpret_cast<uint8_t *>(A.P) + (size_t)board * PIX * 64;
    uint8_t *Vb = reinterpret_cast<uint8_t *>(A.V) + (size_t)board * PIX * 16;
#pragma unroll
    for (int t = 0; t < 2; t++) {
        if (t >= nth || (h && q >= 2)) continue;                     // value head: channels 32..39 only
        const int c0 = (2 * h + t) * 16 + 4 * q;                     // head channel of element 0
        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(A.bh + c0);
#pragma unroll
        for (int nt = 0; nt < 6; nt++) {
            const int p = nt * 16 + r16;
            if (p < PIX) {
                const f32x4 hv = hacc[t][nt];
                const uint2 pk = make_uint2(relu_bf16x2(pack_bf16x2(hv[0] + b4[0], hv[1] + b4[1])),
                                            relu_bf16x2(pack_bf16x2(hv[2] + b4[2], hv[3] + b4[3])));
                if (!h) *reinterpret_cast<uint2 *>(Pb + p * 64 + c0 * 2) = pk;
                else *reinterpret_cast<uint2 *>(Vb + p * 16 + (c0 - 32) * 2) = pk;
            }
        }
    }
    }(lh, lh & 15, lh >> 4);
}

}  // namespace

extern "C" int xq_tower256_mxfp8_nhwc(void *stream, const void *planes, const void *w1, const void *wq, const void *wscale,
                                      const void *bias, const void *wh, const void *bh, void *policy_out, void *value_out,
                                      int n_boards, int n_blocks, const void *row_src_dev, const void *n_rows_dev)
{
    if (!planes || !w1 || !bias || !wh || !bh || !policy_out || !value_out || n_boards <= 0 || n_blocks < 0 ||
        (n_blocks > 0 && (!wq || !wscale)) || n_blocks > 64)
        return XQ_E_INVALID;
    Tower256MxArgs a{ { (const uint16_t *)planes, (const uint16_t *)w1, (const uint16_t *)wq, (const float *)bias,
                        (const uint16_t *)wh, (const float *)bh, (uint16_t *)policy_out, (uint16_t *)value_out, n_boards, n_blocks,
                        nullptr, (const int32_t *)row_src_dev, (const int32_t *)n_rows_dev },
                      (const uint8_t *)wscale };
    if (int rc = tower_lds_opt_in<&k_tower256_mx>(LDS_BYTES_MX256)) return rc;
    hipLaunchKernelGGL(k_tower256_mx, dim3((n_boards + NB - 1) / NB), dim3(256), LDS_BYTES_MX256, reinterpret_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? 0 : XQ_E_HIP;
}
