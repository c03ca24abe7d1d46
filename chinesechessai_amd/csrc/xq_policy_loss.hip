// xq_policy_loss.hip — fused legal-move cross-entropy of the policy head and its gradient.
//
// Reference: trainer.py:324-331 trains the value head only ("策略损失（简化版：只用价值损失）/ 完整版需要把
// move_probs转换为target policy").  This is that full version: the target is the visit distribution pi over a
// position's legal moves (self_play.py:234-239), the prediction is the softmax the search itself applies to the
// logits — over the legal moves only (neural_network.py:148-169) — and the loss of a row is the cross-entropy
//     loss_b = - sum_i pi_i * log p_i,   p = softmax(logits[b][cols[b][0 .. n_moves)])
// The target arrives sparse, as xq_replay_encode_policy_batch writes it: cols int32 [B][128] (policy column of
// every legal move, -1 = unusable), pi float32 [B][128], n_moves int32 [B].
//
// Forward: one wave per row, lane l carries slots l and l + 64 (the convention of the tree kernel's gather sites).
// Backward: d loss_b / d logits[b][c] = p_i - pi_i at the legal columns and 0 elsewhere; the forward leaves the
// sparse residual, the backward writes the dense gradient with every element stored exactly once.
#include "../../include/xq_selfplay.h"
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

enum : int { SLOTS = XQ_MAX_MOVES, GRAD_CHUNK = 2048, GRAD_THREADS = 256 };

// all lanes get the result; the xor butterfly adds / compares in an order that depends on nothing but the lane
// numbers, so a row's result does not depend on the batch or the launch
__device__ __forceinline__ float wave_max(float v)
{
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

__device__ __forceinline__ float wave_sum(float v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(64) void k_policy_loss(const float *logits, int64_t stride, int n_cols, const int32_t *cols,
                                                    const float *pi, const int32_t *n_moves, float *loss, float *resid)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    int n = n_moves[b];
    n = n < 0 ? 0 : (n > SLOTS ? SLOTS : n);
    const size_t row = (size_t)b * SLOTS;
    const int j0 = lane, j1 = lane + 64;
    const int c0 = j0 < n ? cols[row + j0] : -1, c1 = j1 < n ? cols[row + j1] : -1;
    // a column outside the row is as unusable as -1: it is never read
    const bool u0 = c0 >= 0 && c0 < n_cols, u1 = c1 >= 0 && c1 < n_cols;
    const float *x = logits + (size_t)b * (size_t)stride;
    const float x0 = u0 ? x[c0] : 0.f, x1 = u1 ? x[c1] : 0.f;
    const float t0 = u0 ? pi[row + j0] : 0.f, t1 = u1 ? pi[row + j1] : 0.f;
    const float ninf = -__builtin_inff();
    const float mx = wave_max(fmaxf(u0 ? x0 : ninf, u1 ? x1 : ninf));
    float r0 = 0.f, r1 = 0.f, l = 0.f;
    if (mx != ninf) {                                           // (a row with no usable slot: loss 0, residual 0)
        const float d0 = x0 - mx, d1 = x1 - mx;
        const float e0 = u0 ? expf(d0) : 0.f, e1 = u1 ? expf(d1) : 0.f;
        const float sum = wave_sum(e0 + e1);
        const float lg = logf(sum);
        // a term with pi == 0 contributes exactly 0 (never 0 * inf)
        const float a0 = (u0 && t0 != 0.f) ? t0 * (d0 - lg) : 0.f;
        const float a1 = (u1 && t1 != 0.f) ? t1 * (d1 - lg) : 0.f;
        l = -wave_sum(a0 + a1);
        r0 = u0 ? e0 / sum - t0 : 0.f;
        r1 = u1 ? e1 / sum - t1 : 0.f;
    }
    resid[row + j0] = r0;
    resid[row + j1] = r1;
    if (lane == 0) loss[b] = l;
}

// One workgroup builds GRAD_CHUNK consecutive columns of one row in LDS: zero fill | barrier | the row's up to 128
// residuals land on their columns (the columns of a position's legal moves are distinct; should a hand-made target
// name one column twice, its residuals add up, which is the derivative) | barrier | store-out.  Every element of the
// chunk leaves the workgroup in exactly one store, issued after both barriers: nothing in HBM is written twice.
template <bool VEC4>
__global__ __launch_bounds__(GRAD_THREADS) void k_policy_loss_grad(const float *resid, const int32_t *cols, const int32_t *n_moves,
                                                                   const float *scale_dev, float scale_host, float *grad,
                                                                   int64_t stride, int n_cols)
{
    __shared__ __attribute__((aligned(16))) float chunk[GRAD_CHUNK];
    const int b = blockIdx.x, base = blockIdx.y * GRAD_CHUNK, t = threadIdx.x;
    const int len = n_cols - base < GRAD_CHUNK ? n_cols - base : GRAD_CHUNK;       // >= 1 by the grid's size
    for (int i = t; i < GRAD_CHUNK; i += GRAD_THREADS) chunk[i] = 0.f;
    __syncthreads();
    int n = n_moves[b];
    n = n < 0 ? 0 : (n > SLOTS ? SLOTS : n);
    if (t < n) {
        const int c = cols[(size_t)b * SLOTS + t];
        if (c >= base && c < base + len) {
            const float s = scale_dev ? scale_dev[b] : scale_host;
            atomicAdd(&chunk[c - base], s * resid[(size_t)b * SLOTS + t]);
        }
    }
    __syncthreads();
    float *o = grad + (size_t)b * (size_t)stride + base;
    if (VEC4) {                                                 // grad and every row start are 16-byte aligned
        const int len4 = len & ~3;
        for (int i = 4 * t; i < len4; i += 4 * GRAD_THREADS)
            *reinterpret_cast<float4 *>(o + i) = *reinterpret_cast<const float4 *>(chunk + i);
        if (t < len - len4) o[len4 + t] = chunk[len4 + t];
    } else {
        for (int i = t; i < len; i += GRAD_THREADS) o[i] = chunk[i];
    }
}

}  // namespace

static int loss_args_ok(int batch, int n_cols, int64_t stride)
{
    return batch > 0 && n_cols > 0 && stride >= n_cols;
}

extern "C" int xq_policy_loss_f32(void *stream, const void *logits_dev, int64_t row_stride, int n_cols, const void *cols_dev,
                                  const void *pi_dev, const void *n_moves_dev, int batch, void *loss_dev, void *resid_dev)
{
    if (!logits_dev || !cols_dev || !pi_dev || !n_moves_dev || !loss_dev || !resid_dev) return XQ_E_INVALID;
    if (!loss_args_ok(batch, n_cols, row_stride)) return XQ_E_INVALID;
    hipLaunchKernelGGL(k_policy_loss, dim3(batch), dim3(64), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const float *>(logits_dev), row_stride, n_cols, reinterpret_cast<const int32_t *>(cols_dev),
                       reinterpret_cast<const float *>(pi_dev), reinterpret_cast<const int32_t *>(n_moves_dev),
                       reinterpret_cast<float *>(loss_dev), reinterpret_cast<float *>(resid_dev));
    return hipGetLastError() == hipSuccess ? 0 : XQ_E_HIP;
}

extern "C" int xq_policy_loss_grad_f32(void *stream, const void *resid_dev, const void *cols_dev, const void *n_moves_dev,
                                       const void *scale_dev, float scale_host, int batch, void *grad_dev, int64_t row_stride,
                                       int n_cols)
{
    if (!resid_dev || !cols_dev || !n_moves_dev || !grad_dev) return XQ_E_INVALID;
    if (!loss_args_ok(batch, n_cols, row_stride)) return XQ_E_INVALID;
    const dim3 grid(batch, (n_cols + GRAD_CHUNK - 1) / GRAD_CHUNK);
    // 16-byte stores only where every row starts on a 16-byte boundary (8,100 floats = 32,400 B do; an odd stride or
    // a view into a larger tensor may not): otherwise one float per store
    const bool vec4 = (reinterpret_cast<uintptr_t>(grad_dev) % 16 == 0) && (row_stride % 4 == 0);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define XQ_GRAD_ARGS reinterpret_cast<const float *>(resid_dev), reinterpret_cast<const int32_t *>(cols_dev),            \
                     reinterpret_cast<const int32_t *>(n_moves_dev), reinterpret_cast<const float *>(scale_dev), scale_host, \
                     reinterpret_cast<float *>(grad_dev), row_stride, n_cols
    if (vec4) hipLaunchKernelGGL(k_policy_loss_grad<true>, grid, dim3(GRAD_THREADS), 0, s, XQ_GRAD_ARGS);
    else      hipLaunchKernelGGL(k_policy_loss_grad<false>, grid, dim3(GRAD_THREADS), 0, s, XQ_GRAD_ARGS);
#undef XQ_GRAD_ARGS
    return hipGetLastError() == hipSuccess ? 0 : XQ_E_HIP;
}
