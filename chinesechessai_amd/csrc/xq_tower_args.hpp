// xq_tower_args.hpp — what the single-launch trunk kernels of every width (xq_tower.hip: 128 channels,
// xq_tower256.hip: 256 channels, xq_tower192.hip: 192 channels, xq_tower64.hip: 64 channels) share on the host side: the kernel argument block and the per-device opt-in to
// more than 64 KB of dynamic LDS.
#pragma once
#include "../../include/xq_selfplay.h"
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>

namespace xqm {

struct TowerArgs {             // C = 64, 128, 192 or 256 channels
    const uint16_t *planes;    // [G][90][16]
    const uint16_t *w1;        // [9][C][16]
    const uint16_t *wt;        // [2*nblocks][9][C][C]
    const float *bias;         // [1 + 2*nblocks][C]
    const uint16_t *wh;        // [64][C]  (rows 0..31 policy, 32..39 value, rest zero)
    const float *bh;           // [64]
    uint16_t *P;               // [G][90][32]
    uint16_t *V;               // [G][90][8]
    int G, nblocks;
    unsigned long long *stamps;   // diagnostic builds only: 64 u64 per workgroup
    // evaluator row compaction (xq_engine_set_row_compaction), both optional: board b reads the planes of row
    // row_src[b] and only boards below *n_rows exist (device values of the preceding k_assign_rows)
    const int32_t *row_src;
    const int32_t *n_rows;
};

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: remembered per (kernel, device
// ordinal) - a process may drive several GPUs (xq_config.device) - in one atomic bit mask per kernel
template <auto KERNEL>
static int tower_lds_opt_in(int bytes)
{
    static std::atomic<uint64_t> done{ 0 };
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return XQ_E_HIP;
    if (done.load(std::memory_order_acquire) >> dev & 1) return 0;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        return XQ_E_HIP;
    done.fetch_or(1ull << dev, std::memory_order_release);
    return 0;
}

}  // namespace xqm
