// lfgc_bricks.hip -- empty-space skipping for the ray marcher (gfx950): value ranges of bricks of B^3
// cells of the volume lattice, the bricks a transfer function sees nothing in, and the jump of a ray over whole blocks of
// S steps that lie in such bricks.  The model is never evaluated there; lfgc_forward_f32 is not involved.
//   lfgc_brick_minmax_f32     fold an x-slab of lattice values into the (min, max) of every brick that holds one of its planes
//   lfgc_brick_occupancy_f32  brick -> 1 iff the transfer function's extinction is not zero on all of [min - margin, max + margin]
//   lfgc_ray_skip_f32         k_next += S while none of the next S samples of a ray touches an occupied brick
// One writer per brick and per ray, plain vector stores: no atomics, and two runs give the same bits.
// The samples a ray is tested at and the table rows a value falls between are lfgc_ray.h's, as in lfgc_render.hip.
#include "lfgc_ray.h"

namespace {

// ---- ranges -------------------------------------------------------------------------------------------------------------
// Workgroup = the bricks (bx, by, bz0 .. bz0 + nbpb) of one z-chunk.  Thread t owns the z columns z0 + t + 256 m of the
// chunk (one column when B <= 255): it walks the brick's planes and rows that the slab holds, consecutive lanes reading
// consecutive z, and leaves its (min, max) in LDS; thread b then folds the columns of brick bz0 + b with what the table
// holds and writes the pair back.  A NaN counts as (-inf, +inf), which min and max keep.
__global__ __launch_bounds__(kRayBlock) void brick_minmax_kernel(const float* __restrict__ values, int X, int Y, int Z, int x_begin,
                                                                 int x_end, int B, int bx_first, int nby, int nbz, int nbpb,
                                                                 float2* __restrict__ minmax) {
    __shared__ float s_lo[kRayBlock], s_hi[kRayBlock];
    const int t = threadIdx.x;
    const int bx = bx_first + (int)blockIdx.z, by = (int)blockIdx.y, bz0 = (int)blockIdx.x * nbpb;
    const long long Bl = B;
    const int xa = max((int)(bx * Bl), x_begin), xb = min((int)min((bx + 1) * Bl, (long long)X - 1), x_end - 1);
    const int ya = (int)(by * Bl), yb = (int)min((by + 1) * Bl, (long long)Y - 1);
    const long long z0 = bz0 * Bl;
    const long long z_last = min((long long)min(bz0 + nbpb, nbz) * Bl, (long long)Z - 1);      // inclusive
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (long long z = z0 + t; z <= z_last; z += kRayBlock)
        for (int x = xa; x <= xb; ++x)
            for (int y = ya; y <= yb; ++y) {
                const float v = values[((long long)(x - x_begin) * Y + y) * Z + z];
                const bool nan = v != v;
                lo = fminf(lo, nan ? -__builtin_inff() : v);
                hi = fmaxf(hi, nan ? __builtin_inff() : v);
            }
    s_lo[t] = lo;
    s_hi[t] = hi;
    __syncthreads();
    const int bz = bz0 + t;
    if (t < nbpb && bz < nbz) {
        // columns of the brick: local offsets t B .. (t + 1) B of the chunk; with B > 255 the chunk is one brick spread over
        // all threads
        const long long span = z_last - z0;                                                   // last local offset
        const int ia = B <= kRayBlock - 1 ? t * B : 0;
        const int ib = (int)min(B <= kRayBlock - 1 ? (long long)(t + 1) * B : (long long)kRayBlock - 1,
                                min(span, (long long)kRayBlock - 1));
        const long long at = ((long long)bx * nby + by) * nbz + bz;
        float2 mm = minmax[at];
        for (int i = ia; i <= ib; ++i) {
            mm.x = fminf(mm.x, s_lo[i]);
            mm.y = fmaxf(mm.y, s_hi[i]);
        }
        minmax[at] = mm;
    }
}

// ---- occupancy ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRayBlock) void brick_occupancy_kernel(const float2* __restrict__ minmax, long long n_bricks,
                                                                    const float4* __restrict__ tab, int K, float v_min, float tf_scale,
                                                                    float margin, unsigned char* __restrict__ occ) {
    const long long b = (long long)blockIdx.x * kRayBlock + threadIdx.x;
    if (b >= n_bricks) return;
    const float2 mm = minmax[b];
    const float u_max = (float)(K - 1);
    const int i0 = (int)floorf(lfgc_tf_coordinate(mm.x - margin, v_min, tf_scale, u_max));
    const int i1 = (int)ceilf(lfgc_tf_coordinate(mm.y + margin, v_min, tf_scale, u_max));
    bool seen = false;
    for (int i = i0; i <= i1; ++i) seen = seen || tab[i].w != 0.0f;
    occ[b] = seen ? 1 : 0;
}

// ---- skip ---------------------------------------------------------------------------------------------------------------
struct SkipGrid {
    float lo[3], ext[3], cells_f[3];
    int cells[3], nb[3], B;
};

// the two bricks a coordinate can lie in along one axis
__device__ __forceinline__ void brick_pair(float p, const SkipGrid& g, int a, int& b0, int& b1) {
    const float q = (p - g.lo[a]) / g.ext[a] * g.cells_f[a];
    const float top = (float)(g.cells[a] - 1);
    b0 = (int)fminf(fmaxf(floorf(q - LFGC_RAY_SKIP_GUARD), 0.0f), top) / g.B;
    b1 = (int)fminf(fmaxf(floorf(q + LFGC_RAY_SKIP_GUARD), 0.0f), top) / g.B;
}

// A half wave owns a ray, as in the composite kernel: lane l tests sample l of each run of 32, one ballot per run, each
// half reads its own 32 bits.  The halves of a wave leave the loop at different trip counts; nothing here needs the other
// half's lanes (no shuffles), and a ballot counts inactive lanes as 0.
__global__ __launch_bounds__(kRayBlock) void ray_skip_kernel(const int* __restrict__ live, long long n_list, int S,
                                                             const float* __restrict__ origins, const float* __restrict__ dirs,
                                                             const float* __restrict__ t_near, const float* __restrict__ t_far,
                                                             const int* __restrict__ n_steps, int* __restrict__ k_next, float dt,
                                                             const SkipGrid g, const unsigned char* __restrict__ occ,
                                                             int* __restrict__ skipped) {
    const LfgcHalfWave hw;
    if (hw.j >= n_list) return;
    const long long r = live ? live[hw.j] : hw.j;
    const int n = n_steps[r];
    int k0 = k_next[r];
    if (k0 >= n) return;
    const float tn = t_near[r], tf = t_far[r];
    const float ox = origins[r * 3 + 0], oy = origins[r * 3 + 1], oz = origins[r * 3 + 2];
    const float dx = dirs[r * 3 + 0], dy = dirs[r * 3 + 1], dz = dirs[r * 3 + 2];
    int jumped = 0;
    while (k0 < n) {
        bool found = false;                      // the same for all 32 lanes of the half
        for (int s0 = 0; s0 < S && !found; s0 += kRayRun) {
            const int k = k0 + s0 + hw.lane;
            bool touches = false;
            if (k < n) {
                const float tm = lfgc_ray_midpoint(tn, tf, dt, k);
                int x0, x1, y0, y1, z0, z1;
                brick_pair(lfgc_ray_point(ox, dx, tm), g, 0, x0, x1);
                brick_pair(lfgc_ray_point(oy, dy, tm), g, 1, y0, y1);
                brick_pair(lfgc_ray_point(oz, dz, tm), g, 2, z0, z1);
                const long long r00 = ((long long)x0 * g.nb[1] + y0) * g.nb[2], r01 = ((long long)x0 * g.nb[1] + y1) * g.nb[2];
                const long long r10 = ((long long)x1 * g.nb[1] + y0) * g.nb[2], r11 = ((long long)x1 * g.nb[1] + y1) * g.nb[2];
                touches = (occ[r00 + z0] | occ[r00 + z1] | occ[r01 + z0] | occ[r01 + z1] |
                           occ[r10 + z0] | occ[r10 + z1] | occ[r11 + z0] | occ[r11 + z1]) != 0;
            }
            found = hw.ballot(touches) != 0;
        }
        if (found) break;
        k0 += S;
        ++jumped;
    }
    if (hw.lane == 0 && jumped) {
        k_next[r] = k0;
        skipped[r] += jumped;
    }
}

inline int bricks_along(int cells, int B) { return (int)(((long long)cells + B - 1) / B); }

}  // namespace

extern "C" int lfgc_brick_minmax_f32(const float* values, const int32_t* res, int32_t x_begin, int32_t x_end, int32_t B,
                                     float* minmax, lfgc_stream_t stream) {
    if (!values || !res || !minmax) return LFGC_E_NULL;
    const int X = res[0], Y = res[1], Z = res[2];
    if (X < 2 || Y < 2 || Z < 2 || B < 1 || x_begin < 0 || x_end > X || x_begin >= x_end) return LFGC_E_SHAPE;
    if ((uintptr_t)minmax & 7) return LFGC_E_ALIGN;
    const int nbx = bricks_along(X - 1, B), nby = bricks_along(Y - 1, B), nbz = bricks_along(Z - 1, B);
    // brick i holds the planes i B .. min((i + 1) B, X - 1): plane p lies in brick p / B and, on a face, in the one before
    const int bx_first = x_begin % B == 0 && x_begin > 0 ? x_begin / B - 1 : (x_begin / B < nbx ? x_begin / B : nbx - 1);
    const int bx_last = (x_end - 1) / B < nbx ? (x_end - 1) / B : nbx - 1;
    // bricks of one workgroup along z: their columns fit its 256 threads, and the chunks are of about equal size
    const int most = B <= kRayBlock - 1 ? (kRayBlock - 1) / B : 1;
    const int chunks = (nbz + most - 1) / most;
    const int nbpb = (nbz + chunks - 1) / chunks;
    if (nby > 65535 || bx_last - bx_first + 1 > 65535) return LFGC_E_UNSUPPORTED;
    hipLaunchKernelGGL(brick_minmax_kernel, dim3((unsigned)((nbz + nbpb - 1) / nbpb), (unsigned)nby, (unsigned)(bx_last - bx_first + 1)),
                       dim3(kRayBlock), 0, (hipStream_t)stream, values, X, Y, Z, x_begin, x_end, B, bx_first, nby, nbz, nbpb,
                       reinterpret_cast<float2*>(minmax));
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_brick_occupancy_f32(const float* minmax, int64_t n_bricks, const float* tf_table, int K, float v_min,
                                        float tf_scale, float margin, uint8_t* occ, lfgc_stream_t stream) {
    if (!minmax || !tf_table || !occ) return LFGC_E_NULL;
    if (n_bricks < 1 || n_bricks > 0x7fffffffLL || K < 2 || !(tf_scale > 0.0f) || !lfgc_finite(tf_scale) || !lfgc_finite(v_min) ||
        !(margin >= 0.0f) || !lfgc_finite(margin))
        return LFGC_E_SHAPE;
    if (((uintptr_t)minmax & 7) || ((uintptr_t)tf_table & 15)) return LFGC_E_ALIGN;
    hipLaunchKernelGGL(brick_occupancy_kernel, dim3(lfgc_row_grid(n_bricks)), dim3(kRayBlock), 0,
                       (hipStream_t)stream, reinterpret_cast<const float2*>(minmax), (long long)n_bricks,
                       reinterpret_cast<const float4*>(tf_table), K, v_min, tf_scale, margin, occ);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_ray_skip_f32(const int32_t* live, int64_t n_list, const float* origins, const float* dirs, const float* t_near,
                                 const float* t_far, const int32_t* n_steps, int32_t* k_next, float dt, int S, const float* box_min,
                                 const float* box_max, const int32_t* cells, int32_t B, const uint8_t* occ, int32_t* skipped,
                                 lfgc_stream_t stream) {
    if (!origins || !dirs || !t_near || !t_far || !n_steps || !k_next || !box_min || !box_max || !cells || !occ || !skipped)
        return LFGC_E_NULL;
    if (lfgc_ray_list_check(n_list, S, dt) != LFGC_OK || B < 1) return LFGC_E_SHAPE;
    SkipGrid g;
    g.B = B;
    for (int a = 0; a < 3; ++a) {
        if (!(box_min[a] < box_max[a]) || !lfgc_finite(box_min[a]) || !lfgc_finite(box_max[a]) || cells[a] < 1) return LFGC_E_SHAPE;
        g.lo[a] = box_min[a];
        g.ext[a] = box_max[a] - box_min[a];
        g.cells[a] = cells[a];
        g.cells_f[a] = (float)cells[a];
        g.nb[a] = bricks_along(cells[a], B);
    }
    hipLaunchKernelGGL(ray_skip_kernel, dim3(lfgc_half_wave_grid(n_list)), dim3(kRayBlock), 0, (hipStream_t)stream, live,
                       (long long)n_list, S, origins, dirs, t_near, t_far, n_steps, k_next, dt, g, occ, skipped);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}
