// lfgc_ssim.hip -- structural similarity of two fp32 arrays (n0, n1, n2) over separable, valid-only windows (gfx950,
// DESIGN.md 3.4.1).  One kernel serves volumes (w, w, w) and images viewed as (C, height, width) with windows (1, w, w).
//   lfgc_ssim_workspace_bytes   bytes of the per-workgroup partials, 0 for refused arguments
//   lfgc_ssim_planes_f32        plane_sums[i0] = sum of the SSIM of the windows (i0, ., .); optionally the map itself
// A workgroup owns one origin plane i0 and a tile of (T1, T2) windows of the other two axes, one window per thread.  Per
// tap t0 it stages the tile's input plane o0 + t0 of both arrays, halo included, as (x, y) pairs in LDS and every thread
// adds g0[t0] * (its window's weighted sums over t1, t2) to five fp64 moments.  The tile shape depends on (w, s) only and the
// tile count on (n1, n2, w, s) only; the tile's values are folded by a fixed tree into workspace[i0 * ntiles + tile] and a
// second kernel folds a plane's tiles in a fixed order: no floating-point atomics, and a plane sum has the same bits
// whatever n0 is, i.e. wherever the caller cut the slab that holds the plane.
#include "lfgc_common.h"

#pragma clang fp contract(off)      // 2 mu mu against mu mu + mu mu must round alike: products are never fused into sums

namespace {

constexpr int kSsimBlock = 256;
constexpr int kSsimMaxWindow = 16;
constexpr int kSsimTile1 = 8;                     // windows of a tile along axis 1 ...
constexpr int kSsimTile2 = 32;                    // ... and along axis 2: one per thread
constexpr int kSsimMaxPairs = 7680;               // (x, y) pairs of a staged plane: 60 KB of dynamic LDS + 2 KB static
constexpr int kSsimFoldBlock = 64;

struct SsimPlan {
    double g[3 * kSsimMaxWindow];                 // weights, axis a at g + off[a]
    double c1, c2, k;
    long long n1, n2, m0, m1, m2;
    long long tiles1, tiles2, ntiles;
    int off[3], w[3], s[3];
    int T1, T2;                                   // windows of a tile
    int ls1, ls2;                                 // LDS distance of neighbouring windows: min(s, w), gaps are not staged
    int E1, E2;                                   // staged extent: (T - 1) ls + w
};

// Shape arguments only: everything the workspace size depends on.  g, c1, c2, k are left alone.
int ssim_plan(int n0, int n1, int n2, const int* w, const int* s, SsimPlan& p) {
    if (!w || !s) return LFGC_E_NULL;
    const int n[3] = {n0, n1, n2};
    for (int a = 0; a < 3; ++a)
        if (w[a] < 1 || s[a] < 1 || n[a] < w[a]) return LFGC_E_SHAPE;
    for (int a = 0; a < 3; ++a)
        if (w[a] > kSsimMaxWindow) return LFGC_E_UNSUPPORTED;
    if ((long long)n1 * n2 > (1LL << 61) / n0) return LFGC_E_UNSUPPORTED;      // element offsets stay far inside int64
    for (int a = 0; a < 3; ++a) {
        p.w[a] = w[a];
        p.s[a] = s[a];
    }
    p.off[0] = 0;
    p.off[1] = w[0];
    p.off[2] = w[0] + w[1];
    p.n1 = n1;
    p.n2 = n2;
    p.m0 = (n0 - w[0]) / s[0] + 1;
    p.m1 = (n1 - w[1]) / s[1] + 1;
    p.m2 = (n2 - w[2]) / s[2] + 1;
    p.ls1 = s[1] < w[1] ? s[1] : w[1];
    p.ls2 = s[2] < w[2] ? s[2] : w[2];
    p.T1 = kSsimTile1;
    p.T2 = kSsimTile2;
    for (;;) {                                    // a function of (w, s) alone; T1 = T2 = 1 stages at most 256 pairs
        p.E1 = (p.T1 - 1) * p.ls1 + w[1];
        p.E2 = (p.T2 - 1) * p.ls2 + w[2];
        if (p.E1 * p.E2 <= kSsimMaxPairs) break;
        if (p.T1 > 1) p.T1 >>= 1; else p.T2 >>= 1;
    }
    p.tiles1 = (p.m1 + p.T1 - 1) / p.T1;
    p.tiles2 = (p.m2 + p.T2 - 1) / p.T2;
    p.ntiles = p.tiles1 * p.tiles2;               // < 2^62
    if (p.ntiles > 0x7fffffffLL / p.m0) return LFGC_E_UNSUPPORTED;             // one workgroup per (plane, tile): a 1-D grid
    return LFGC_OK;
}

// Offset of staged element e of an axis from the tile's first input element: contiguous while windows touch or overlap,
// else window e / w, tap e % w.
__device__ __forceinline__ long long ssim_src(int e, int w, int s) { return s <= w ? (long long)e : (long long)(e / w) * s + e % w; }

__global__ __launch_bounds__(kSsimBlock) void ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, SsimPlan p,
                                                               double* __restrict__ partials, double* __restrict__ map) {
    extern __shared__ __align__(16) float2 s_xy[];
    __shared__ double s_red[kSsimBlock];
    const int tid = threadIdx.x;
    const long long i0 = blockIdx.x / p.ntiles;
    const long long tile = blockIdx.x % p.ntiles;
    const long long tile1 = tile / p.tiles2, tile2 = tile % p.tiles2;
    const long long base1 = tile1 * p.T1 * p.s[1], base2 = tile2 * p.T2 * p.s[2];     // first input row / column of the tile
    const int j1 = tid / p.T2, j2 = tid % p.T2;
    const long long i1 = tile1 * p.T1 + j1, i2 = tile2 * p.T2 + j2;
    const bool active = j1 < p.T1 && i1 < p.m1 && i2 < p.m2;
    const int pairs = p.E1 * p.E2;
    const double* g0 = p.g + p.off[0];
    const double* g1 = p.g + p.off[1];
    const double* g2 = p.g + p.off[2];
    const float2* mine = s_xy + (long long)(j1 * p.ls1) * p.E2 + j2 * p.ls2;

    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};    // mu_x, mu_y, E_xx, E_yy, E_xy
    for (int t0 = 0; t0 < p.w[0]; ++t0) {
        const long long plane = (i0 * p.s[0] + t0) * p.n1;
        for (int e = tid; e < pairs; e += kSsimBlock) {
            const int e1 = e / p.E2, e2 = e % p.E2;
            const long long y = base1 + ssim_src(e1, p.w[1], p.s[1]);
            const long long z = base2 + ssim_src(e2, p.w[2], p.s[2]);
            float2 v = make_float2(0.0f, 0.0f);   // past the array: only windows that do not exist read it
            if (y < p.n1 && z < p.n2) {
                const long long at = (plane + y) * p.n2 + z;
                v = make_float2(a[at], b[at]);
            }
            s_xy[e] = v;
        }
        __syncthreads();
        if (active) {
            double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
            for (int t1 = 0; t1 < p.w[1]; ++t1) {
                const float2* row = mine + t1 * p.E2;
                double r[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
                for (int t2 = 0; t2 < p.w[2]; ++t2) {
                    const float2 v = row[t2];
                    const double x = (double)v.x, y = (double)v.y, gz = g2[t2];
                    r[0] = fma(gz, x, r[0]);
                    r[1] = fma(gz, y, r[1]);
                    r[2] = fma(gz, x * x, r[2]);  // fp32 x fp32 is exact in fp64; the three second moments take the same
                    r[3] = fma(gz, y * y, r[3]);  // operations, so equal inputs give equal bits
                    r[4] = fma(gz, x * y, r[4]);
                }
                const double gy = g1[t1];
                for (int i = 0; i < 5; ++i) q[i] = fma(gy, r[i], q[i]);
            }
            const double gx = g0[t0];
            for (int i = 0; i < 5; ++i) acc[i] = fma(gx, q[i], acc[i]);
        }
        __syncthreads();
    }

    double ssim = 0.0;
    if (active) {
        const double mx = acc[0], my = acc[1];
        const double mxx = mx * mx, myy = my * my, mxy = mx * my;
        const double vx = p.k * (acc[2] - mxx), vy = p.k * (acc[3] - myy), vxy = p.k * (acc[4] - mxy);
        const double num = (2.0 * mxy + p.c1) * (2.0 * vxy + p.c2);
        const double den = ((mxx + myy) + p.c1) * ((vx + vy) + p.c2);
        ssim = num / den;
        if (map) map[(i0 * p.m1 + i1) * p.m2 + i2] = ssim;
    }
    s_red[tid] = ssim;                            // a window that does not exist adds +0.0: exact
    __syncthreads();
    for (int h = kSsimBlock / 2; h > 0; h >>= 1) {
        if (tid < h) s_red[tid] += s_red[tid + h];
        __syncthreads();
    }
    if (tid == 0) partials[blockIdx.x] = s_red[0];
}

// plane_sums[i0] = the plane's tile partials: lane l adds the tiles l, l + 64, ... in that order, then a fixed tree.
__global__ __launch_bounds__(kSsimFoldBlock) void ssim_fold_kernel(const double* __restrict__ partials, long long ntiles,
                                                                  double* __restrict__ plane_sums) {
    __shared__ double s_red[kSsimFoldBlock];
    const int tid = threadIdx.x;
    const double* mine = partials + (long long)blockIdx.x * ntiles;
    double sum = 0.0;
    for (long long t = tid; t < ntiles; t += kSsimFoldBlock) sum += mine[t];
    s_red[tid] = sum;
    __syncthreads();
    for (int h = kSsimFoldBlock / 2; h > 0; h >>= 1) {
        if (tid < h) s_red[tid] += s_red[tid + h];
        __syncthreads();
    }
    if (tid == 0) plane_sums[blockIdx.x] = s_red[0];
}

}  // namespace

extern "C" int64_t lfgc_ssim_workspace_bytes(int n0, int n1, int n2, const int* w, const int* s) {
    SsimPlan p;
    if (ssim_plan(n0, n1, n2, w, s, p) != LFGC_OK) return 0;
    return (int64_t)(p.m0 * p.ntiles) * (int64_t)sizeof(double);
}

extern "C" int lfgc_ssim_planes_f32(const float* a, const float* b, int n0, int n1, int n2, const double* weights, const int* w,
                                    const int* s, double c1, double c2, double cov_norm, double* plane_sums, double* map,
                                    void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!a || !b || !weights || !w || !s || !plane_sums || !workspace) return LFGC_E_NULL;
    SsimPlan p;
    const int code = ssim_plan(n0, n1, n2, w, s, p);
    if (code != LFGC_OK) return code;
    if (!(c1 > 0.0) || !(c2 > 0.0) || !(cov_norm > 0.0) || c1 * 0.0 != 0.0 || c2 * 0.0 != 0.0 || cov_norm * 0.0 != 0.0)
        return LFGC_E_SHAPE;                      // positive and finite: the denominator of equal inputs cannot vanish
    const int taps = w[0] + w[1] + w[2];
    for (int t = 0; t < taps; ++t) {
        if (weights[t] * 0.0 != 0.0) return LFGC_E_SHAPE;
        p.g[t] = weights[t];
    }
    for (int t = taps; t < 3 * kSsimMaxWindow; ++t) p.g[t] = 0.0;
    p.c1 = c1;
    p.c2 = c2;
    p.k = cov_norm;
    const long long blocks = p.m0 * p.ntiles;
    if (workspace_bytes < blocks * (long long)sizeof(double)) return LFGC_E_WORKSPACE;
    if (((uintptr_t)plane_sums | (uintptr_t)map | (uintptr_t)workspace) & 7) return LFGC_E_ALIGN;
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)blocks), dim3(kSsimBlock), (size_t)p.E1 * p.E2 * sizeof(float2),
                       (hipStream_t)stream, a, b, p, partials, map);
    LFGC_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(ssim_fold_kernel, dim3((unsigned)p.m0), dim3(kSsimFoldBlock), 0, (hipStream_t)stream,
                       (const double*)partials, p.ntiles, plane_sums);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}
