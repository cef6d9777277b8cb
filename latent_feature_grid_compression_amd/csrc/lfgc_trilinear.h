// lfgc_trilinear.h -- the one definition of grid_sample's trilinear cell (ATen GridSampler.h, align_corners=False, zero
// padding), per axis.  Every kernel that samples the feature grid or scatters into it takes its geometry from here:
// LfgcSampler::issue and LfgcColumnSampler::stage_a (lfgc_forward.h), lfgc_bwd_data_kernel and the deferred scatter
// (lfgc_bwd_data.h).  Forward and backward agree bit for bit because they run these operations in this order.
// What stays with the caller, because it fixes the caller's rounding and instruction stream: how offsets are formed
// (32-bit byte offsets in the forward, long long float offsets in the backward), whether weights are zeroed per axis
// (forward) or per corner (backward), the corner order dz = c >> 2, dy = (c >> 1) & 1, dx = c & 1 and the product
// order (wx wy) wz.
#pragma once
#include <hip/hip_runtime.h>

struct LfgcAxisCell {
    int i0, size;              // lower cell index, clamped to [-2, size]; the axis length
    float w[2];                // weights of cells i0 and i0 + 1, NOT masked: a cell outside the grid counts as zero (inside())

    __device__ __forceinline__ bool inside(int d) const { return (unsigned)(i0 + d) < (unsigned)size; }
    __device__ __forceinline__ int clamped(int d) const { return min(max(i0 + d, 0), size - 1); }   // a row that can be read
};

// p in [-1, 1] spans the axis; grid_sampler_unnormalize: ((p + 1) * size - 1) / 2, one rounding per operation.
__device__ __forceinline__ LfgcAxisCell lfgc_axis_cell(float p, int size) {
    const float ip = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(p, 1.0f), (float)size), 1.0f), 0.5f);
    const float f0 = floorf(ip);
    LfgcAxisCell c;
    // clamped to [-2, size] before the conversion: absurd / NaN positions stay defined (fmaxf(NaN, -2) = -2), and both
    // cells of such an axis are then outside by the index test alone
    c.i0 = (int)fminf(fmaxf(f0, -2.0f), (float)size);
    c.size = size;
    c.w[1] = __fsub_rn(ip, f0);
    c.w[0] = __fsub_rn(__fadd_rn(f0, 1.0f), ip);
    return c;
}
