// lfgc_render.hip -- direct volume rendering around the network evaluation (gfx950): everything a ray marcher needs
// except the values themselves, which come from lfgc_forward_f32 / lfgc_input_gradient_f32 unchanged.
//   lfgc_ray_clip_f32        slab test of every ray against the volume's box -> [t_near, t_far], number of steps
//   lfgc_ray_samples_f32     the next S sample positions of every live ray, S consecutive rows per ray: one 32-sample
//                            tile of the forward kernel is 32 consecutive steps of ONE ray
//   lfgc_ray_composite_f32   transfer function, headlight shading and front-to-back compositing of those S samples
//                            into the per-ray state (premultiplied r, g, b and the transmittance T)
//   lfgc_ray_composite2d_f32 the same under a 2-D table over value and gradient magnitude
//   lfgc_ray_composite_preint_f32  the same with pre-integrated classification: slabs between consecutive samples
//   lfgc_ray_compact         order-preserving list of the rays that still have steps left and are not yet opaque
//   lfgc_ray_iso_scan_f32    first-hit isosurface: the first sign change of v - iso among those S samples -> a bracket
//   lfgc_ray_iso_refine_f32  one bisection step of every bracket, and the position of the next trial
//   lfgc_ray_iso_finish_f32  one secant step inside the final bracket: depth and position of the hit
// All arithmetic is fp32 in the order include/lfgc.h states (the build has no contraction and correctly rounded
// division), so the clip and the positions can be restated bit for bit on the host.  One writer per ray: no atomics.
// Segments, sample points, the table coordinate and the half wave that owns a ray are lfgc_ray.h's.
#include "lfgc_ray.h"
#include "lfgc_select.h"

namespace {

struct RayBox { float lo[3], hi[3]; };

// ---- clip -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRayBlock) void ray_clip_kernel(const float* __restrict__ origins, const float* __restrict__ dirs,
                                                             long long n_rays, const RayBox box, float t_min, float t_max, float dt,
                                                             int max_steps, float* __restrict__ t_near, float* __restrict__ t_far,
                                                             int* __restrict__ n_steps) {
    const long long r = (long long)blockIdx.x * kRayBlock + threadIdx.x;
    if (r >= n_rays) return;
    float tn = t_min, tf = t_max;
    bool hit = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float o = origins[r * 3 + a], d = dirs[r * 3 + a];
        if (d == 0.0f) {
            if (!(box.lo[a] <= o && o <= box.hi[a])) hit = false;
        } else {
            const float inv = 1.0f / d;
            const float t1 = (box.lo[a] - o) * inv;
            const float t2 = (box.hi[a] - o) * inv;
            tn = fmaxf(tn, fminf(t1, t2));
            tf = fminf(tf, fmaxf(t1, t2));
        }
    }
    hit = hit && tf > tn;
    int n = 0;
    if (hit) {
        const float q = ceilf((tf - tn) / dt);
        n = q >= (float)max_steps ? max_steps : (int)q;          // the comparison also keeps the conversion in range
    } else {
        tn = tf = t_min;                                         // a miss: the empty interval
    }
    t_near[r] = tn;
    t_far[r] = tf;
    n_steps[r] = n;
}

// ---- samples --------------------------------------------------------------------------------------------------------
// thread = one output row; the 12-byte rows of a wave are consecutive, so its three stores cover 768 contiguous bytes
__global__ __launch_bounds__(kRayBlock) void ray_samples_kernel(const int* __restrict__ live, long long n_rows, int S,
                                                                const float* __restrict__ origins, const float* __restrict__ dirs,
                                                                const float* __restrict__ t_near, const float* __restrict__ t_far,
                                                                const int* __restrict__ n_steps, const int* __restrict__ k_next,
                                                                float dt, float* __restrict__ pos) {
    const long long row = (long long)blockIdx.x * kRayBlock + threadIdx.x;
    if (row >= n_rows) return;
    const long long j = row / S;
    const int s = (int)(row - j * S);
    const long long r = live[j];
    int k = k_next[r] + s;
    const int n = n_steps[r];
    if (k > n - 1) k = n - 1;                    // padding rows repeat the last valid sample
    if (k < 0) k = 0;
    const float tm = lfgc_ray_midpoint(t_near[r], t_far[r], dt, k);
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[row * 3 + c] = lfgc_ray_point(origins, dirs, r, c, tm);
}

// ---- composite ------------------------------------------------------------------------------------------------------
// A half wave (32 lanes) owns one ray and walks its S samples in runs of 32: lane l of the half reads value l of the run
// (one coalesced 128-byte row), forms its own alpha and colour, and the run is folded with a log-step product scan of the
// (1 - alpha) factors and a butterfly sum of the contributions.  T never increases, so the samples that contribute are a
// prefix of the run: T after the run is T before the first lane that does not contribute.  The lanes a ray's samples sit
// on do not depend on the list the ray is in, so neither does a single bit of its result.
// TF2D: the table is (K, Kg) over value and gradient magnitude (lfgc_tf_lookup2d) -- the lookup is the only difference.
template <bool SHADE, bool TF2D>
__global__ __launch_bounds__(kRayBlock) void ray_composite_kernel(const int* __restrict__ live, long long n_live, int S,
                                                                  const float* __restrict__ values, const float* __restrict__ grad,
                                                                  const float* __restrict__ dirs, const float* __restrict__ t_near,
                                                                  const float* __restrict__ t_far, const int* __restrict__ n_steps,
                                                                  int* __restrict__ k_next, float dt,
                                                                  const float4* __restrict__ tab, int K, int Kg, float v_min,
                                                                  float tf_scale, float g_scale, float opacity_limit, float ka,
                                                                  float kd, float4* __restrict__ state) {
    const LfgcHalfWave hw;
    if (hw.j >= n_live) return;                  // a whole half wave leaves: the shuffles below stay inside one half
    const long long r = live[hw.j];
    const float tn = t_near[r], tf = t_far[r];
    const int n = n_steps[r], k0 = k_next[r];
    float dx = 0.0f, dy = 0.0f, dz = 0.0f;
    if (SHADE) { dx = dirs[r * 3 + 0]; dy = dirs[r * 3 + 1]; dz = dirs[r * 3 + 2]; }
    const float4 st = state[r];
    float cr = st.x, cg = st.y, cb = st.z, T = st.w;
    for (int s0 = 0; s0 < S; s0 += kRayRun) {
        const long long row = hw.j * S + s0 + hw.lane;
        const int k = k0 + s0 + hw.lane;
        float alpha = 0.0f, er = 0.0f, eg = 0.0f, eb = 0.0f;
        if (k < n) {
            float a, b;
            lfgc_ray_segment(tn, tf, dt, k, a, b);
            const float len = fmaxf(b - a, 0.0f);        // a step count rounded up: the last segment starts an ulp past t_far
            float gx = 0.0f, gy = 0.0f, gz = 0.0f, gn = 0.0f;
            if (SHADE || TF2D) {
                gx = grad[row * 3 + 0]; gy = grad[row * 3 + 1]; gz = grad[row * 3 + 2];
                gn = lfgc_grad_norm(gx, gy, gz);
            }
            const float4 rgba = TF2D ? lfgc_tf_lookup2d(tab, K, Kg, values[row], gn, v_min, tf_scale, g_scale)
                                     : lfgc_tf_lookup(tab, K, values[row], v_min, tf_scale);
            alpha = 1.0f - expf(-rgba.w * len);
            float shade = 1.0f;
            if (SHADE) shade = gn > 0.0f ? ka + kd * fabsf(gx * dx + gy * dy + gz * dz) / gn : ka + kd;
            const float w = alpha * shade;
            er = w * rgba.x;
            eg = w * rgba.y;
            eb = w * rgba.z;
        }
        float incl = 1.0f - alpha;               // inclusive product of the factors of lanes 0..lane
#pragma unroll
        for (int off = 1; off < kRayRun; off <<= 1) {
            const float t = __shfl_up(incl, off, kRayRun);
            if (hw.lane >= off) incl *= t;
        }
        float excl = __shfl_up(incl, 1, kRayRun);
        if (hw.lane == 0) excl = 1.0f;
        const float t_before = T * excl;
        // the first lane that is out ends the ray (the rounded products of two scan trees need not be ordered, so the
        // prefix is cut there explicitly); T after the run: T before that lane, else T times every factor
        const unsigned long long out_mask = hw.ballot(!(1.0f - t_before < opacity_limit));
        const int first_out = LfgcHalfWave::first(out_mask);
        const bool in = hw.lane < first_out;
        float sr = in ? t_before * er : 0.0f, sg = in ? t_before * eg : 0.0f, sb = in ? t_before * eb : 0.0f;
#pragma unroll
        for (int off = kRayRun / 2; off > 0; off >>= 1) {
            sr += __shfl_xor(sr, off, kRayRun);
            sg += __shfl_xor(sg, off, kRayRun);
            sb += __shfl_xor(sb, off, kRayRun);
        }
        const float t_all = T * __shfl(incl, kRayRun - 1, kRayRun);
        const float t_cut = __shfl(t_before, first_out & (kRayRun - 1), kRayRun);
        T = out_mask ? t_cut : t_all;
        cr += sr; cg += sg; cb += sb;
    }
    if (hw.lane == 0) {
        state[r] = make_float4(cr, cg, cb, T);
        k_next[r] = k0 + S;
    }
}

// ---- composite, pre-integrated ----------------------------------------------------------------------------------------
// The same half wave, runs, product scan, cut and butterfly sum as ray_composite_kernel; what a lane folds is the SLAB
// between its sample and the one before it (lfgc_tf_slab_mean over the two table coordinates) instead of its segment.
// Lane l sees its predecessor's value through a shuffle, lane 0 takes the previous run's lane 31 or the carry
// (carry_v, carry_k: the ray's last value and its step; valid iff carry_k == k_next - 1), as ray_iso_scan_kernel does.
// A sample without a composited predecessor opens with the half slab from its segment's front; the ray's last sample
// also folds the closing half slab to t_far into its own lane.  No LDS.
template <bool SHADE>
__global__ __launch_bounds__(kRayBlock) void ray_composite_preint_kernel(const int* __restrict__ live, long long n_live, int S,
                                                                         const float* __restrict__ values, const float* __restrict__ grad,
                                                                         const float* __restrict__ dirs, const float* __restrict__ t_near,
                                                                         const float* __restrict__ t_far, const int* __restrict__ n_steps,
                                                                         int* __restrict__ k_next, float dt,
                                                                         const float4* __restrict__ tab, const double* __restrict__ pre,
                                                                         int K, float v_min, float tf_scale, float opacity_limit,
                                                                         float ka, float kd, float4* __restrict__ state,
                                                                         float* __restrict__ carry_v, int* __restrict__ carry_k) {
    const LfgcHalfWave hw;
    if (hw.j >= n_live) return;                  // a whole half wave leaves: the shuffles below stay inside one half
    const long long r = live[hw.j];
    const float tn = t_near[r], tf = t_far[r];
    const int n = n_steps[r], k0 = k_next[r];
    float dx = 0.0f, dy = 0.0f, dz = 0.0f;
    if (SHADE) { dx = dirs[r * 3 + 0]; dy = dirs[r * 3 + 1]; dz = dirs[r * 3 + 2]; }
    const float4 st = state[r];
    float cr = st.x, cg = st.y, cb = st.z, T = st.w;
    float last = carry_v[r];
    bool has_last = k0 > 0 && carry_k[r] == k0 - 1;      // a jump of the skip kernel moved k_next: the carry is stale
    const float u_max = (float)(K - 1);
    for (int s0 = 0; s0 < S; s0 += kRayRun) {
        const long long row = hw.j * S + s0 + hw.lane;
        const int k = k0 + s0 + hw.lane;
        const float v = values[row];
        float prev = __shfl_up(v, 1, kRayRun);
        if (hw.lane == 0) prev = last;
        float factor = 1.0f, er = 0.0f, eg = 0.0f, eb = 0.0f;
        if (k < n) {
            const bool joined = hw.lane > 0 || has_last;
            float len, len_close;
            lfgc_ray_slab(tn, tf, dt, k, joined, len, len_close);
            const float u = lfgc_tf_coordinate(v, v_min, tf_scale, u_max);
            const float4 m = lfgc_tf_slab_mean(tab, pre, K, joined ? lfgc_tf_coordinate(prev, v_min, tf_scale, u_max) : u, u);
            const float alpha = 1.0f - expf(-m.w * len);
            float shade = 1.0f;
            if (SHADE) {
                const float gx = grad[row * 3 + 0], gy = grad[row * 3 + 1], gz = grad[row * 3 + 2];
                const float gn = lfgc_grad_norm(gx, gy, gz);
                shade = gn > 0.0f ? ka + kd * fabsf(gx * dx + gy * dy + gz * dz) / gn : ka + kd;
            }
            const float w = alpha * shade;
            er = w * m.x;
            eg = w * m.y;
            eb = w * m.z;
            factor = 1.0f - alpha;
            if (k == n - 1) {                    // the closing half slab behind the ray's last sample, in the same lane
                const float4 c = lfgc_tf_slab_mean(tab, pre, K, u, u);
                const float alpha2 = 1.0f - expf(-c.w * len_close);
                const float w2 = (factor * alpha2) * shade;
                er += w2 * c.x;
                eg += w2 * c.y;
                eb += w2 * c.z;
                factor *= 1.0f - alpha2;
            }
            if (k == n - 1 || s0 + hw.lane == S - 1) {   // the ray's last row of this call with k < n: one lane
                carry_v[r] = v;
                carry_k[r] = k;
            }
        }
        float incl = factor;                     // inclusive product of the factors of lanes 0..lane
#pragma unroll
        for (int off = 1; off < kRayRun; off <<= 1) {
            const float t = __shfl_up(incl, off, kRayRun);
            if (hw.lane >= off) incl *= t;
        }
        float excl = __shfl_up(incl, 1, kRayRun);
        if (hw.lane == 0) excl = 1.0f;
        const float t_before = T * excl;
        // the cut at the first lane that is out, as in ray_composite_kernel
        const unsigned long long out_mask = hw.ballot(!(1.0f - t_before < opacity_limit));
        const int first_out = LfgcHalfWave::first(out_mask);
        const bool in = hw.lane < first_out;
        float sr = in ? t_before * er : 0.0f, sg = in ? t_before * eg : 0.0f, sb = in ? t_before * eb : 0.0f;
#pragma unroll
        for (int off = kRayRun / 2; off > 0; off >>= 1) {
            sr += __shfl_xor(sr, off, kRayRun);
            sg += __shfl_xor(sg, off, kRayRun);
            sb += __shfl_xor(sb, off, kRayRun);
        }
        const float t_all = T * __shfl(incl, kRayRun - 1, kRayRun);
        const float t_cut = __shfl(t_before, first_out & (kRayRun - 1), kRayRun);
        T = out_mask ? t_cut : t_all;
        cr += sr; cg += sg; cb += sb;
        last = __shfl(v, kRayRun - 1, kRayRun);
        has_last = true;
    }
    if (hw.lane == 0) {
        state[r] = make_float4(cr, cg, cb, T);
        k_next[r] = k0 + S;
    }
}

// ---- order-preserving list of the rays still worth marching -----------------------------------------------------------
// the selection of lfgc_select.h over ray ids: the item is the ray, the sink appends it
struct RayAlive {
    typedef int Item;
    const int* prev;             // previous list (ascending ray ids) or NULL = every ray 0..n-1
    const int* n_steps;
    const int* k_next;
    const float4* state;
    float opacity_limit;
    __device__ __forceinline__ bool operator()(long long i, long long n, int& ray) const {
        ray = 0;
        if (i >= n) return false;
        ray = prev ? prev[i] : (int)i;
        return k_next[ray] < n_steps[ray] && 1.0f - state[ray].w < opacity_limit;
    }
};

struct RayListSink {
    int* live_out;
    __device__ __forceinline__ void operator()(long long, long long, bool flag, long long rank, const int& ray) const {
        if (flag) live_out[rank] = ray;
    }
};

// ---- isosurface: the first sign change of v - iso along a ray, its bisection and the hit point ---------------------------
// inside(v) is lfgc_iso_inside: v - iso >= 0.  The scan has the composite kernel's form: a half wave owns a ray and
// walks its S values in runs of 32; lane l sees its predecessor through a shuffle, lane 0 takes the value carried in
// state.x (the last value of the ray's previous block; meaningful iff k_next > 0) or the previous run's lane 31.  The
// first crossing of the half's 32 ballot bits ends the ray: its lane writes the bracket, state.w = 0 and k_next = k.
__global__ __launch_bounds__(kRayBlock) void ray_iso_scan_kernel(const int* __restrict__ live, long long n_live, int S,
                                                                 const float* __restrict__ values, const float* __restrict__ t_near,
                                                                 const float* __restrict__ t_far, const int* __restrict__ n_steps,
                                                                 int* __restrict__ k_next, float dt, float iso,
                                                                 float4* __restrict__ state, float4* __restrict__ bracket) {
    const LfgcHalfWave hw;
    if (hw.j >= n_live) return;                  // a whole half wave leaves: the shuffles below stay inside one half
    const long long r = live[hw.j];
    const int n = n_steps[r], k0 = k_next[r];
    float last = state[r].x;
    for (int s0 = 0; s0 < S; s0 += kRayRun) {
        const int k = k0 + s0 + hw.lane;
        const float v = values[hw.j * S + s0 + hw.lane];
        float prev = __shfl_up(v, 1, kRayRun);
        if (hw.lane == 0) prev = last;
        const bool cross = k >= 1 && k < n && lfgc_iso_inside(prev, iso) != lfgc_iso_inside(v, iso);     // k < n: no padding row
        const unsigned long long mask = hw.ballot(cross);
        if (mask) {                              // the same for all 32 lanes of the half
            if (hw.lane == LfgcHalfWave::first(mask)) {
                const float tn = t_near[r], tf = t_far[r];
                bracket[r] = make_float4(lfgc_ray_midpoint(tn, tf, dt, k - 1), lfgc_ray_midpoint(tn, tf, dt, k), prev - iso, v - iso);
                state[r] = make_float4(v, 0.0f, 0.0f, 0.0f);
                k_next[r] = k;
            }
            return;
        }
        last = __shfl(v, kRayRun - 1, kRayRun);
    }
    if (hw.lane == 0) {
        state[r] = make_float4(last, 0.0f, 0.0f, 1.0f);
        k_next[r] = k0 + S;
    }
}

// thread = one bracketed ray of the list: fold the value at the bracket's midpoint in (if given), emit the next midpoint
__global__ __launch_bounds__(kRayBlock) void ray_iso_refine_kernel(const int* __restrict__ list, long long n,
                                                                   const float* __restrict__ values, const float* __restrict__ origins,
                                                                   const float* __restrict__ dirs, float iso,
                                                                   float4* __restrict__ bracket, float* __restrict__ pos) {
    const long long j = (long long)blockIdx.x * kRayBlock + threadIdx.x;
    if (j >= n) return;
    const long long r = list[j];
    float4 br = bracket[r];
    if (values) {
        const float tm = 0.5f * (br.x + br.y);
        const float f = values[j] - iso;
        if ((f >= 0.0f) == (br.z >= 0.0f)) { br.x = tm; br.z = f; }
        else { br.y = tm; br.w = f; }
        bracket[r] = br;
    }
    const float tm = 0.5f * (br.x + br.y);
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[j * 3 + c] = lfgc_ray_point(origins, dirs, r, c, tm);
}

// thread = one bracketed ray of the list: one secant step inside the final bracket
__global__ __launch_bounds__(kRayBlock) void ray_iso_finish_kernel(const int* __restrict__ list, long long n,
                                                                   const float* __restrict__ origins, const float* __restrict__ dirs,
                                                                   const float4* __restrict__ bracket, float* __restrict__ t_hit,
                                                                   float* __restrict__ pos) {
    const long long j = (long long)blockIdx.x * kRayBlock + threadIdx.x;
    if (j >= n) return;
    const long long r = list[j];
    const float4 br = bracket[r];
    const float q = br.z / (br.z - br.w);
    float t = br.x + (br.y - br.x) * q;
    if (!(q - q == 0.0f)) t = 0.5f * (br.x + br.y);
    t = fminf(fmaxf(t, br.x), br.y);
    t_hit[j] = t;
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[j * 3 + c] = lfgc_ray_point(origins, dirs, r, c, t);
}

}  // namespace

extern "C" int lfgc_ray_clip_f32(const float* origins, const float* dirs, int64_t n_rays, const float* box_min, const float* box_max,
                                 float t_min, float t_max, float dt, int max_steps, float* t_near, float* t_far, int32_t* n_steps,
                                 lfgc_stream_t stream) {
    if (!origins || !dirs || !box_min || !box_max || !t_near || !t_far || !n_steps) return LFGC_E_NULL;
    if (n_rays < 1 || n_rays > 0x7fffffffLL || max_steps < 1 || !(dt > 0.0f) || !lfgc_finite(dt) || !lfgc_finite(t_min))
        return LFGC_E_SHAPE;
    RayBox box;
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = box_min[a];
        box.hi[a] = box_max[a];
        if (!(box.lo[a] <= box.hi[a])) return LFGC_E_SHAPE;
    }
    hipLaunchKernelGGL(ray_clip_kernel, dim3(lfgc_row_grid(n_rays)), dim3(kRayBlock), 0, (hipStream_t)stream,
                       origins, dirs, (long long)n_rays, box, t_min, t_max, dt, max_steps, t_near, t_far, n_steps);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_ray_samples_f32(const int32_t* live, int64_t n_live, const float* origins, const float* dirs, const float* t_near,
                                    const float* t_far, const int32_t* n_steps, const int32_t* k_next, float dt, int S, float* pos,
                                    lfgc_stream_t stream) {
    if (!live || !origins || !dirs || !t_near || !t_far || !n_steps || !k_next || !pos) return LFGC_E_NULL;
    if (lfgc_ray_list_check(n_live, S, dt) != LFGC_OK) return LFGC_E_SHAPE;
    const long long n_rows = (long long)n_live * S;
    const unsigned nblocks = lfgc_row_grid(n_rows);
    if (!nblocks) return LFGC_E_UNSUPPORTED;
    hipLaunchKernelGGL(ray_samples_kernel, dim3(nblocks), dim3(kRayBlock), 0, (hipStream_t)stream, live, n_rows, S, origins,
                       dirs, t_near, t_far, n_steps, k_next, dt, pos);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_ray_composite_f32(const int32_t* live, int64_t n_live, const float* values, const float* grad, const float* dirs,
                                      const float* t_near, const float* t_far, const int32_t* n_steps, int32_t* k_next, float dt,
                                      int S, const float* tf_table, int K, float v_min, float tf_scale, float opacity_limit, float ka,
                                      float kd, float* state, lfgc_stream_t stream) {
    if (!live || !values || !dirs || !t_near || !t_far || !n_steps || !k_next || !tf_table || !state) return LFGC_E_NULL;
    if (lfgc_ray_list_check(n_live, S, dt) != LFGC_OK || K < 2) return LFGC_E_SHAPE;
    if (((uintptr_t)tf_table | (uintptr_t)state) & 15) return LFGC_E_ALIGN;
    hipLaunchKernelGGL((grad ? ray_composite_kernel<true, false> : ray_composite_kernel<false, false>),
                       dim3(lfgc_half_wave_grid(n_live)), dim3(kRayBlock), 0, (hipStream_t)stream, live, (long long)n_live, S, values,
                       grad, dirs, t_near, t_far, n_steps, k_next, dt, reinterpret_cast<const float4*>(tf_table), K, 0, v_min,
                       tf_scale, 0.0f, opacity_limit, ka, kd, reinterpret_cast<float4*>(state));
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_ray_composite2d_f32(const int32_t* live, int64_t n_live, const float* values, const float* grad, const float* dirs,
                                        const float* t_near, const float* t_far, const int32_t* n_steps, int32_t* k_next, float dt,
                                        int S, const float* tf_table, int Kv, int Kg, float v_min, float tf_scale, float g_scale,
                                        int shade, float opacity_limit, float ka, float kd, float* state, lfgc_stream_t stream) {
    if (!live || !values || !grad || !dirs || !t_near || !t_far || !n_steps || !k_next || !tf_table || !state) return LFGC_E_NULL;
    if (lfgc_ray_list_check(n_live, S, dt) != LFGC_OK || Kv < 2 || Kg < 2 || (long long)Kv * Kg > (1LL << 22) ||
        !(g_scale > 0.0f) || !lfgc_finite(g_scale) || (shade != 0 && shade != 1))
        return LFGC_E_SHAPE;
    if (((uintptr_t)tf_table | (uintptr_t)state) & 15) return LFGC_E_ALIGN;
    hipLaunchKernelGGL((shade ? ray_composite_kernel<true, true> : ray_composite_kernel<false, true>),
                       dim3(lfgc_half_wave_grid(n_live)), dim3(kRayBlock), 0, (hipStream_t)stream, live, (long long)n_live, S, values,
                       grad, dirs, t_near, t_far, n_steps, k_next, dt, reinterpret_cast<const float4*>(tf_table), Kv, Kg, v_min,
                       tf_scale, g_scale, opacity_limit, ka, kd, reinterpret_cast<float4*>(state));
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_ray_composite_preint_f32(const int32_t* live, int64_t n_live, const float* values, const float* grad,
                                             const float* dirs, const float* t_near, const float* t_far, const int32_t* n_steps,
                                             int32_t* k_next, float dt, int S, const float* tf_table, int K, float v_min,
                                             float tf_scale, float opacity_limit, float ka, float kd, float* state,
                                             const double* pre, float* carry_v, int32_t* carry_k, lfgc_stream_t stream) {
    if (!live || !values || !dirs || !t_near || !t_far || !n_steps || !k_next || !tf_table || !state || !pre || !carry_v || !carry_k)
        return LFGC_E_NULL;
    if (lfgc_ray_list_check(n_live, S, dt) != LFGC_OK || K < 2 || K > (1 << 22)) return LFGC_E_SHAPE;
    if (((uintptr_t)tf_table | (uintptr_t)pre | (uintptr_t)state) & 15) return LFGC_E_ALIGN;
    hipLaunchKernelGGL((grad ? ray_composite_preint_kernel<true> : ray_composite_preint_kernel<false>),
                       dim3(lfgc_half_wave_grid(n_live)), dim3(kRayBlock), 0, (hipStream_t)stream, live, (long long)n_live, S, values,
                       grad, dirs, t_near, t_far, n_steps, k_next, dt, reinterpret_cast<const float4*>(tf_table), pre, K, v_min,
                       tf_scale, opacity_limit, ka, kd, reinterpret_cast<float4*>(state), carry_v, carry_k);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int64_t lfgc_ray_compact_workspace_bytes(int64_t n) { return lfgc_select_workspace(n); }

extern "C" int lfgc_ray_compact(const int32_t* prev, int64_t n_prev, const int32_t* n_steps, const int32_t* k_next, const float* state,
                                float opacity_limit, int32_t* live_out, int64_t* count, void* workspace, int64_t workspace_bytes,
                                lfgc_stream_t stream) {
    if (!n_steps || !k_next || !state || !live_out || !count || !workspace) return LFGC_E_NULL;
    if (n_prev < 1 || n_prev > 0x7fffffffLL) return LFGC_E_SHAPE;
    if ((uintptr_t)state & 15) return LFGC_E_ALIGN;
    const RayAlive alive = {prev, n_steps, k_next, reinterpret_cast<const float4*>(state), opacity_limit};
    return lfgc_select(alive, RayListSink{live_out}, n_prev, reinterpret_cast<long long*>(count), workspace, workspace_bytes,
                       (hipStream_t)stream);
}

extern "C" int lfgc_ray_iso_scan_f32(const int32_t* live, int64_t n_live, const float* values, const float* t_near, const float* t_far,
                                     const int32_t* n_steps, int32_t* k_next, float dt, int S, float iso, float* state, float* bracket,
                                     lfgc_stream_t stream) {
    if (!live || !values || !t_near || !t_far || !n_steps || !k_next || !state || !bracket) return LFGC_E_NULL;
    if (lfgc_ray_list_check(n_live, S, dt) != LFGC_OK || !lfgc_finite(iso)) return LFGC_E_SHAPE;
    if (((uintptr_t)state | (uintptr_t)bracket) & 15) return LFGC_E_ALIGN;
    hipLaunchKernelGGL(ray_iso_scan_kernel, dim3(lfgc_half_wave_grid(n_live)), dim3(kRayBlock), 0, (hipStream_t)stream, live,
                       (long long)n_live, S, values, t_near, t_far, n_steps, k_next, dt, iso, reinterpret_cast<float4*>(state),
                       reinterpret_cast<float4*>(bracket));
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_ray_iso_refine_f32(const int32_t* list, int64_t n, const float* values, const float* origins, const float* dirs,
                                       float iso, float* bracket, float* pos, lfgc_stream_t stream) {
    if (!list || !origins || !dirs || !bracket || !pos) return LFGC_E_NULL;
    if (n < 1 || n > 0x7fffffffLL || !lfgc_finite(iso)) return LFGC_E_SHAPE;
    if ((uintptr_t)bracket & 15) return LFGC_E_ALIGN;
    hipLaunchKernelGGL(ray_iso_refine_kernel, dim3(lfgc_row_grid(n)), dim3(kRayBlock), 0, (hipStream_t)stream, list,
                       (long long)n, values, origins, dirs, iso, reinterpret_cast<float4*>(bracket), pos);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_ray_iso_finish_f32(const int32_t* list, int64_t n, const float* origins, const float* dirs, const float* bracket,
                                       float* t_hit, float* pos, lfgc_stream_t stream) {
    if (!list || !origins || !dirs || !bracket || !t_hit || !pos) return LFGC_E_NULL;
    if (n < 1 || n > 0x7fffffffLL) return LFGC_E_SHAPE;
    if ((uintptr_t)bracket & 15) return LFGC_E_ALIGN;
    hipLaunchKernelGGL(ray_iso_finish_kernel, dim3(lfgc_row_grid(n)), dim3(kRayBlock), 0, (hipStream_t)stream, list,
                       (long long)n, origins, dirs, reinterpret_cast<const float4*>(bracket), t_hit, pos);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}
