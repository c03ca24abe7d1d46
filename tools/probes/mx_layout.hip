// What csrc/xq_tower_mx.hip relies on, asked of the device (one wave):
//   1. v_cvt_pk_fp8_f32 at and above 448 (the kernel's quantiser never hands it such a value);
//   2. v_mfma_scale_f32_16x16x128_f8f6f4, both operands e4m3: which byte of a lane's 8 operand registers meets which byte
//      of the other operand (A row i carries bit i of a byte's position, B column 0 is one-hot: D[0..6][0] spells the
//      position of the A byte it met), and which lane's scale byte governs it (A row 0 / B column 0 all ones, the scale of
//      lane quarter s doubled: D[0][0] = 2 where s governs).  Position = (lane >> 4) * 32 + register * 4 + byte.
//   hipcc --offload-arch=gfx950 -O2 -o mx_layout tools/probes/mx_layout.hip && ./mx_layout
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

template <class F> __device__ i32x8 frag(int q, F one)            // byte (register r, byte b) = 1.0 (0x38) where one(position)
{
    i32x8 v;
    for (int r = 0; r < 8; r++) {
        unsigned w = 0;
        for (int b = 0; b < 4; b++) w |= one(q * 32 + r * 4 + b) ? 0x38u << (8 * b) : 0u;
        v[r] = (int)w;
    }
    return v;
}

__global__ __launch_bounds__(64) void k(unsigned *cvt, const float *cvt_in, int n_cvt, int *met, int *gov_a, int *gov_b)
{
    const int lane = threadIdx.x, i = lane & 15, q = lane >> 4;
    if (lane < n_cvt) cvt[lane] = (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(cvt_in[lane], -cvt_in[lane], 0, false) & 0xffffu;
    const f32x4 z = { 0.f, 0.f, 0.f, 0.f };
    for (int pos = 0; pos < 128; pos++) {
        const i32x8 hot = frag(q, [&](int p) { return i == 0 && p == pos; });
        const i32x8 ones = frag(q, [&](int) { return i == 0; });
        const i32x8 bits = frag(q, [&](int p) { return i < 7 && ((p >> i) & 1); });
        f32x4 d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bits, hot, z, 0, 0, 0, 127, 0, 127);
        int code = 0;                                               // lane 0: rows 0..3 of column 0, lane 16: rows 4..7
        for (int e = 0; e < 4; e++) code |= (d[e] != 0.f) << (4 * q + e);
        if (i == 0 && q < 2) atomicOr(&met[pos], code);
        for (int s = 0; s < 4; s++) {
            d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ones, hot, z, 0, 0, 0, q == s ? 128 : 127, 0, 127);
            if (lane == 0 && d[0] == 2.f) gov_a[pos] = s;           // A's scale, B one-hot at pos
            d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(hot, ones, z, 0, 0, 0, 127, 0, q == s ? 128 : 127);
            if (lane == 0 && d[0] == 2.f) gov_b[pos] = s;           // B's scale, A one-hot at pos
        }
    }
}

int main()
{
    const float in[] = { 416.f, 432.f, 447.f, 448.f, 449.f, 463.f, 464.f, 465.f, 480.f, 1024.f, 1e30f };
    const int n = sizeof in / sizeof in[0];
    unsigned *cvt; float *cin; int *res, h[3 * 128];
    unsigned hc[16];
    hipMalloc(&cvt, 64 * 4); hipMalloc(&cin, sizeof in); hipMalloc(&res, sizeof h);
    hipMemcpy(cin, in, sizeof in, hipMemcpyHostToDevice);
    memset(h, 0, sizeof h);
    for (int p = 128; p < 384; p++) h[p] = -1;
    hipMemcpy(res, h, sizeof h, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, cvt, cin, n, res, res + 128, res + 256);
    if (hipMemcpy(h, res, sizeof h, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hc, cvt, n * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        printf("HIP error\n");
        return 1;
    }
    for (int j = 0; j < n; j++) printf("cvt_pk_fp8_f32(%g, %g) -> 0x%02x 0x%02x\n", in[j], -in[j], hc[j] & 0xff, hc[j] >> 8);
    int same = 0;
    for (int p = 0; p < 128; p++) same += h[p] == p;
    printf("a byte of B meets the byte of A at the same (lane quarter, register, byte): %d of 128 positions\n", same);
    for (int q = 0; q < 4; q++)
        for (int half = 0; half < 2; half++) {
            int ga = h[128 + q * 32 + half * 16], gb = h[256 + q * 32 + half * 16], uniform = 1;
            for (int j = 0; j < 16; j++) uniform &= h[128 + q * 32 + half * 16 + j] == ga && h[256 + q * 32 + half * 16 + j] == gb;
            printf("lane quarter %d registers %d..%d: scale of lane quarter A %d, B %d%s\n", q, half * 4, half * 4 + 3, ga, gb,
                   uniform ? "" : " (NOT uniform over the 16 bytes)");
        }
    return 0;
}
