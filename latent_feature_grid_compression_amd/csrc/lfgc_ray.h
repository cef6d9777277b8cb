// lfgc_ray.h -- where a ray's samples are defined (gfx950), once, for lfgc_render.hip, lfgc_bricks.hip and
// lfgc_mesh.hip: the skip kernel looks at the positions the samples kernel writes and sees a value's table rows as the
// composite kernel does by construction.  fp32 in the order include/lfgc.h states, one rounding per operation.
#pragma once
#include "lfgc_common.h"

constexpr int kRayBlock = 256;                  // threads per workgroup of the ray and brick kernels
constexpr int kRayRun = 32;                     // samples of one ray handled per step: one half wave

// segment k of a ray: [a, b] with a = tn + k dt (never an accumulated sum) and b = min(a + dt, tf)
__device__ __forceinline__ void lfgc_ray_segment(float tn, float tf, float dt, int k, float& a, float& b) {
    a = tn + (float)k * dt;
    b = fminf(a + dt, tf);
}
__device__ __forceinline__ float lfgc_ray_midpoint(float tn, float tf, float dt, int k) {      // the parameter of sample k
    float a, b;
    lfgc_ray_segment(tn, tf, dt, k, a, b);
    return 0.5f * (a + b);
}

// one component of the point o + t d, and component c of it for row r of the (R, 3) tables
__device__ __forceinline__ float lfgc_ray_point(float o, float d, float t) { return o + t * d; }
__device__ __forceinline__ float lfgc_ray_point(const float* origins, const float* dirs, long long r, int c, float t) {
    return lfgc_ray_point(origins[r * 3 + c], dirs[r * 3 + c], t);
}

// A half wave (32 lanes) owns entry j of a ray list and walks the ray's samples in runs of kRayRun, lane l on sample l of
// the run.  A kernel leaves with `if (hw.j >= n) return;` before its first shuffle or ballot: a whole half leaves together.
struct LfgcHalfWave {
    int lane;
    long long j;
    __device__ __forceinline__ LfgcHalfWave()
        : lane(threadIdx.x & (kRayRun - 1)), j((long long)blockIdx.x * (kRayBlock / kRayRun) + (threadIdx.x / kRayRun)) {}
    __device__ __forceinline__ unsigned long long ballot(bool p) const {      // this half's 32 bits; an inactive lane counts as 0
        return (__ballot(p) >> ((threadIdx.x & 32) ? 32 : 0)) & 0xffffffffull;
    }
    // the first set lane of such a mask, or kRayRun
    __device__ __forceinline__ static int first(unsigned long long mask) { return mask ? __ffsll((long long)mask) - 1 : kRayRun; }
};

__device__ __forceinline__ bool lfgc_iso_inside(float v, float iso) { return v - iso >= 0.0f; }      // a NaN is not inside

// the row coordinate of value v in a transfer-function table of u_max + 1 rows
__device__ __forceinline__ float lfgc_tf_coordinate(float v, float v_min, float tf_scale, float u_max) {
    return fminf(fmaxf((v - v_min) * tf_scale, 0.0f), u_max);
}

// the cell i = min((int)u, K - 2) of such a coordinate in a table of K rows and the fraction f = u - i inside it
__device__ __forceinline__ void lfgc_tf_cell(float u, int K, int& i, float& f) {
    i = (int)u;
    if (i > K - 2) i = K - 2;
    f = u - (float)i;
}
__device__ __forceinline__ float4 lfgc_tf_lerp(const float4& c0, const float4& c1, float f) {
    return make_float4(c0.x + f * (c1.x - c0.x), c0.y + f * (c1.y - c0.y), c0.z + f * (c1.z - c0.z), c0.w + f * (c1.w - c0.w));
}
// rgba of value v in a 1-D table of K rows
__device__ __forceinline__ float4 lfgc_tf_lookup(const float4* __restrict__ tab, int K, float v, float v_min, float tf_scale) {
    int i;
    float f;
    lfgc_tf_cell(lfgc_tf_coordinate(v, v_min, tf_scale, (float)(K - 1)), K, i, f);
    return lfgc_tf_lerp(tab[i], tab[i + 1], f);
}
// ---- pre-integrated classification (include/lfgc.h: lfgc_ray_composite_preint_f32) -----------------------------------------
// the bracket B(c; x0, x1) of the cell between rows t0 and t1, 0 <= x0 <= x1 <= 1: the mean over the cell fractions
// [x0, x1] of (tau r, tau g, tau b, tau), tau and the colour both linear in the fraction.  No cancellation where x0 is
// close to x1; at x0 == x1 the pointwise lookup
__device__ __forceinline__ float4 lfgc_tf_bracket(const float4& t0, const float4& t1, float x0, float x1) {
    const float s = x0 + x1;
    const float q3 = ((x0 * x0 + x0 * x1) + x1 * x1) / 3.0f;
    const float dx = t1.x - t0.x, dy = t1.y - t0.y, dz = t1.z - t0.z, dw = t1.w - t0.w;
    return make_float4((t0.w * t0.x + (0.5f * (t0.w * dx + dw * t0.x)) * s) + (dw * dx) * q3,
                       (t0.w * t0.y + (0.5f * (t0.w * dy + dw * t0.y)) * s) + (dw * dy) * q3,
                       (t0.w * t0.z + (0.5f * (t0.w * dz + dw * t0.z)) * s) + (dw * dz) * q3,
                       t0.w + (0.5f * dw) * s);
}
// the slab between the table coordinates u_a and u_b (either order): its extinction-weighted mean colour in x, y, z and
// its mean extinction in w.  pre (K, 4) float64: row i = the sum of B(c; 0, 1) over the cells c < i
__device__ __forceinline__ float4 lfgc_tf_slab_mean(const float4* __restrict__ tab, const double* __restrict__ pre, int K,
                                                    float u_a, float u_b) {
    int i_lo, i_hi;
    float f_lo, f_hi;
    lfgc_tf_cell(fminf(u_a, u_b), K, i_lo, f_lo);
    lfgc_tf_cell(fmaxf(u_a, u_b), K, i_hi, f_hi);
    float4 m;
    float tau;
    if (i_lo == i_hi) {
        m = lfgc_tf_bracket(tab[i_lo], tab[i_lo + 1], f_lo, f_hi);
        tau = m.w;
    } else {                                     // the rest of the low cell, the whole cells between, the start of the high cell
        const float w_lo = 1.0f - f_lo;          // > 0: f_lo == 1 only in the last cell, and then both are in it
        const float4 lo = lfgc_tf_bracket(tab[i_lo], tab[i_lo + 1], f_lo, 1.0f);
        const float4 hi = lfgc_tf_bracket(tab[i_hi], tab[i_hi + 1], 0.0f, f_hi);
        const double* p1 = pre + 4 * (long long)i_hi;
        const double* p0 = pre + 4 * (long long)(i_lo + 1);
        m = make_float4((w_lo * lo.x + (float)(p1[0] - p0[0])) + f_hi * hi.x, (w_lo * lo.y + (float)(p1[1] - p0[1])) + f_hi * hi.y,
                        (w_lo * lo.z + (float)(p1[2] - p0[2])) + f_hi * hi.z, (w_lo * lo.w + (float)(p1[3] - p0[3])) + f_hi * hi.w);
        tau = m.w / ((w_lo + (float)(i_hi - i_lo - 1)) + f_hi);
    }
    const bool lit = m.w > 0.0f;
    return make_float4(lit ? m.x / m.w : 0.0f, lit ? m.y / m.w : 0.0f, lit ? m.z / m.w : 0.0f, tau);
}
// the lengths of the slabs sample k owns: its own, [t_m(k-1), t_m(k)] where it is joined to a composited sample k - 1 and
// else the opening half [a_k, t_m(k)], and the closing half [t_m(k), b_k] (which counts for the ray's last sample alone)
__device__ __forceinline__ void lfgc_ray_slab(float tn, float tf, float dt, int k, bool joined, float& len, float& len_close) {
    float a, b;
    lfgc_ray_segment(tn, tf, dt, k, a, b);
    const float tm = 0.5f * (a + b);
    len = fmaxf(tm - (joined ? lfgc_ray_midpoint(tn, tf, dt, k - 1) : a), 0.0f);
    len_close = fmaxf(b - tm, 0.0f);
}

// the cell (i, j) and the fractions (f, h) of value v and gradient magnitude gn in a row-major (Kv, Kg) table whose g axis
// starts at 0: a NaN of either lands in row 0 of its axis (fmaxf)
__device__ __forceinline__ void lfgc_tf_cell2d(int Kv, int Kg, float v, float gn, float v_min, float tf_scale, float g_scale,
                                               int& i, float& f, int& j, float& h) {
    lfgc_tf_cell(lfgc_tf_coordinate(v, v_min, tf_scale, (float)(Kv - 1)), Kv, i, f);
    lfgc_tf_cell(lfgc_tf_coordinate(gn, 0.0f, g_scale, (float)(Kg - 1)), Kg, j, h);
}
// rgba of (v, gn) in such a table, entry tab[i * Kg + j]: along the value in both g rows, then along g
__device__ __forceinline__ float4 lfgc_tf_lookup2d(const float4* __restrict__ tab, int Kv, int Kg, float v, float gn, float v_min,
                                                   float tf_scale, float g_scale) {
    int i, j;
    float f, h;
    lfgc_tf_cell2d(Kv, Kg, v, gn, v_min, tf_scale, g_scale, i, f, j, h);
    const float4* row = tab + (long long)i * Kg + j;
    const float4 lo = lfgc_tf_lerp(row[0], row[Kg], f);
    const float4 hi = lfgc_tf_lerp(row[1], row[Kg + 1], f);
    return lfgc_tf_lerp(lo, hi, h);
}
// |g| as the shading and the tables form it
__device__ __forceinline__ float lfgc_grad_norm(float gx, float gy, float gz) { return sqrtf(gx * gx + gy * gy + gz * gz); }

// ---- host side of the entries ---------------------------------------------------------------------------------------------
inline bool lfgc_finite(float v) { return v - v == 0.0f; }

// a launch over a list of n rays with S samples each at step dt: LFGC_OK or the argument error
inline int lfgc_ray_list_check(int64_t n, int S, float dt) {
    return n < 1 || n > 0x7fffffffLL || S < kRayRun || S % kRayRun != 0 || !(dt > 0.0f) ? LFGC_E_SHAPE : LFGC_OK;
}
// workgroups of a launch with one half wave per list entry
inline unsigned lfgc_half_wave_grid(int64_t n) { return (unsigned)((n + kRayBlock / kRayRun - 1) / (kRayBlock / kRayRun)); }
// workgroups of a launch with one thread per row (n_rows >= 1), or 0 where that takes more than 2^31 - 1 of them
inline unsigned lfgc_row_grid(long long n_rows) {
    const long long nblocks = (n_rows + kRayBlock - 1) / kRayBlock;
    return nblocks > 0x7fffffffLL ? 0u : (unsigned)nblocks;
}
