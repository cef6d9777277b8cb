// lfgc_histogram.hip -- joint histogram of value and gradient magnitude (gfx950): the tool a 2-D transfer
// function is designed with.  Bin (i, j) of a sample is the table cell lfgc_ray_composite2d_f32 would interpolate in for a
// table of (Bv + 1, Bg + 1) rows -- lfgc_ray.h's cell, the same fp32 operations.
//   lfgc_joint_histogram_f32  counts (Bv, Bg) int64 += the samples' bins
// One LDS histogram of 32-bit counters per workgroup, flushed with 64-bit integer atomics, non-zero bins only: integer sums,
// so the counts depend neither on scheduling nor on how the samples are cut into calls.
#include "lfgc_ray.h"

namespace {

constexpr int kHistMaxBins = 16384;               // 64 KB of LDS
constexpr int kHistMaxGrid = 1024;                // workgroups of a launch, as the other grid-stride row kernels
constexpr long long kHistMaxRows = 1LL << 31;     // rows per workgroup: its 32-bit counters cannot overflow

__global__ __launch_bounds__(kRayBlock) void joint_histogram_kernel(const float* __restrict__ values, const float* __restrict__ grad,
                                                                    long long n, int Bv, int Bg, float v_min, float v_scale,
                                                                    float g_scale, unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned int s_hist[];
    const int bins = Bv * Bg;
    for (int b = threadIdx.x; b < bins; b += kRayBlock) s_hist[b] = 0u;
    __syncthreads();
    for (long long row = (long long)blockIdx.x * kRayBlock + threadIdx.x; row < n; row += (long long)gridDim.x * kRayBlock) {
        const float gn = lfgc_grad_norm(grad[row * 3 + 0], grad[row * 3 + 1], grad[row * 3 + 2]);
        int i, j;
        float f, h;
        lfgc_tf_cell2d(Bv + 1, Bg + 1, values[row], gn, v_min, v_scale, g_scale, i, f, j, h);
        atomicAdd(&s_hist[i * Bg + j], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += kRayBlock) {
        const unsigned int c = s_hist[b];
        if (c) atomicAdd(&counts[b], (unsigned long long)c);
    }
}

}  // namespace

extern "C" int lfgc_joint_histogram_f32(const float* values, const float* grad, int64_t n, int Bv, int Bg, float v_min, float v_scale,
                                        float g_scale, int64_t* counts, lfgc_stream_t stream) {
    if (!values || !grad || !counts) return LFGC_E_NULL;
    if (n < 0 || Bv < 1 || Bg < 1 || !lfgc_finite(v_min) || !(v_scale > 0.0f) || !lfgc_finite(v_scale) || !(g_scale > 0.0f) ||
        !lfgc_finite(g_scale))
        return LFGC_E_SHAPE;
    if ((long long)Bv * Bg > kHistMaxBins) return LFGC_E_UNSUPPORTED;
    if ((uintptr_t)counts & 7) return LFGC_E_ALIGN;
    if (n == 0) return LFGC_OK;
    const long long blocks = (n + kRayBlock - 1) / kRayBlock;
    long long grid = blocks < kHistMaxGrid ? blocks : kHistMaxGrid;
    const long long least = (n + kHistMaxRows - 1) / kHistMaxRows;       // a workgroup sees at most ceil(blocks / grid) * 256 rows
    if (grid < least) grid = least;
    if (grid > 0x7fffffffLL) return LFGC_E_UNSUPPORTED;
    hipLaunchKernelGGL(joint_histogram_kernel, dim3((unsigned)grid), dim3(kRayBlock), (size_t)Bv * Bg * sizeof(unsigned int),
                       (hipStream_t)stream, values, grad, (long long)n, Bv, Bg, v_min, v_scale, g_scale,
                       reinterpret_cast<unsigned long long*>(counts));
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}
