// lfgc_backward.hip -- C-ABI entry for the backward of the fused path: checks, workspace carving, dispatch; and the
// backward's kernels that are no templates (the fixed-point scatter's passes, the slab reduction), compiled here once.
#include <cstdlib>
#include "lfgc_backward.h"
#include "lfgc_f16split.h"       // u32x4

typedef int LfgcBwdDispatch(int MT, const LfgcBwdArgs& a, const LfgcWgradArgs& w, int waves, int precision, int lds_bytes,
                            int grid_data, int grid_w, hipStream_t stream, const LfgcDetScatter* det);
LfgcBwdDispatch lfgc_bwd_dispatch_ch8, lfgc_bwd_dispatch_ch16, lfgc_bwd_dispatch_ch24, lfgc_bwd_dispatch_ch32;
typedef int LfgcIgradDispatch(int MT, const LfgcBwdArgs& a, int waves, int precision, int lds_bytes, int grid_data, hipStream_t stream);
LfgcIgradDispatch lfgc_igrad_dispatch_ch8, lfgc_igrad_dispatch_ch16, lfgc_igrad_dispatch_ch24, lfgc_igrad_dispatch_ch32;

#ifdef LFGC_STAMPS
static unsigned long long* g_bwd_stamps = nullptr;
// Diagnostics builds only (tools/phase_stamps.py bwd): device buffer of 20 counters per wave slot of the data kernel.
extern "C" void lfgc_debug_set_bwd_stamp_buffer(void* p) { g_bwd_stamps = reinterpret_cast<unsigned long long*>(p); }
#endif

// ---- the fixed-point scatter's passes around lfgc_bwd_scatter_det_kernel (lfgc_backward.h has the scheme) ----------------
static __global__ __launch_bounds__(256) void lfgc_det_zero_kernel(long long* __restrict__ acc, long long cells,
                                                                 unsigned* __restrict__ maxw) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;            // cells is a multiple of 8
    if (i < cells) *reinterpret_cast<u32x4*>(acc + i) = u32x4{0u, 0u, 0u, 0u};
    if (blockIdx.x == 0 && threadIdx.x == 0) *maxw = 0u;
}

static __global__ __launch_bounds__(256) void lfgc_det_max_kernel(const float* __restrict__ dfeat, long long count,
                                                                unsigned* __restrict__ maxw) {
    unsigned m = 0u;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const unsigned b = __float_as_uint(dfeat[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(maxw, m);
}

int lfgc_launch_det_max(const float* dfeat, long long count, unsigned* maxw, hipStream_t stream) {
    const long long mblocks = (count + 255) / 256;
    hipLaunchKernelGGL(lfgc_det_max_kernel, dim3((unsigned)(mblocks < 2048 ? mblocks : 2048)), dim3(256), 0, stream, dfeat, count, maxw);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

static __global__ __launch_bounds__(256) void lfgc_det_finish_kernel(const long long* __restrict__ acc,
                                                                   const unsigned* __restrict__ maxw, long long n,
                                                                   float* __restrict__ d_grid, long long cells) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;            // cells is a multiple of 8
    if (i >= cells) return;
    const unsigned mb = *maxw;
    f32x4 o;
    if (mb >= kLfgcDetNonFinite) {
        o.x = o.y = o.z = o.w = __uint_as_float(0x7fc00000u);
    } else {
        const double q = lfgc_det_pow2(lfgc_det_qexp(mb, n));                      // max == 0: acc is all zero
        o.x = (float)((double)acc[i] * q); o.y = (float)((double)acc[i + 1] * q);
        o.z = (float)((double)acc[i + 2] * q); o.w = (float)((double)acc[i + 3] * q);
    }
    *reinterpret_cast<f32x4*>(d_grid + i) = o;
}

// ---- the slab reduction (kernel 3 of lfgc_backward.h) ----------------------------------------------------------------------
struct LfgcReduceArgs {
    const float* slabs;
    int nslabs, slab_floats;
    float* dw[LFGC_MAX_LAYERS + 1];
    float* db[LFGC_MAX_LAYERS + 1];
    LfgcPlan plan;
    int col_of_src[64];        // layer 0: packed column that holds original column c
};

// d_weights / d_biases in nn.Linear layout = sum over workgroup slabs.  A block owns 64 consecutive output
// elements; its 4 waves each sum a quarter of the slabs (coalesced 256-B rows), the quarters are combined in a
// fixed order through LDS, so the result is bitwise repeatable.
static __global__ __launch_bounds__(256) void lfgc_bwd_reduce_kernel(const LfgcReduceArgs a) {
    const LfgcPlan& p = a.plan;
    const int K0 = p.E + p.C;
    const int n0 = p.H * K0 + p.H;                     // layer 0: weights then bias
    const int n1 = p.H * p.H + p.H;
    const int total = n0 + (p.L - 1) * n1 + p.H + 1;
    __shared__ float part[4][64];
    const int o = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int idx = blockIdx.x * 64 + o;
    int src = 0;
    float* dst = nullptr;
    if (idx < total) {
        if (idx < n0) {
            if (idx < p.H * K0) {
                const int row = idx / K0, c = idx % K0;
                src = row * p.K0R + a.col_of_src[c];
                dst = a.dw[0] + idx;
            } else {
                const int r = idx - p.H * K0;
                src = p.HP * p.K0R + r;
                dst = a.db[0] + r;
            }
        } else if (idx < n0 + (p.L - 1) * n1) {
            const int l = 1 + (idx - n0) / n1, oo = (idx - n0) % n1;
            const int base = lfgc_slab_layer_off(p, l);
            if (oo < p.H * p.H) {
                src = base + (oo / p.H) * p.HP + (oo % p.H);
                dst = a.dw[l] + oo;
            } else {
                src = base + p.HP * p.HP + (oo - p.H * p.H);
                dst = a.db[l] + (oo - p.H * p.H);
            }
        } else {
            const int oo = idx - n0 - (p.L - 1) * n1;
            const int base = lfgc_slab_layer_off(p, p.L);
            if (oo < p.H) { src = base + oo; dst = a.dw[p.L] + oo; }
            else { src = base + p.HP; dst = a.db[p.L]; }
        }
    }
    float s = 0.0f;
    if (idx < total) {
        const float* sp = a.slabs + src;
        for (int g = q; g < a.nslabs; g += 4) s += sp[(long long)g * a.slab_floats];
    }
    part[q][o] = s;
    __syncthreads();
    if (q == 0 && idx < total) *dst = ((part[0][o] + part[1][o]) + part[2][o]) + part[3][o];
}

namespace {
#ifndef LFGC_MAX_SLABS
#define LFGC_MAX_SLABS 256
#endif
const int kMaxSlabs = LFGC_MAX_SLABS;   // workgroups of the weight-gradient kernel (one partial slab each)
// The per-channel instantiation files' entries, by CH / 8 - 1 (CH = 8, 16, 24, 32: lfgc_mlp_supported).
LfgcBwdDispatch* const kBwd[4] = {lfgc_bwd_dispatch_ch8, lfgc_bwd_dispatch_ch16, lfgc_bwd_dispatch_ch24, lfgc_bwd_dispatch_ch32};
LfgcIgradDispatch* const kIgrad[4] = {lfgc_igrad_dispatch_ch8, lfgc_igrad_dispatch_ch16, lfgc_igrad_dispatch_ch24, lfgc_igrad_dispatch_ch32};

struct Carve {
    long long ntiles, nbatches;
    int nslabs;                // partial slabs = tile groups of the weight-gradient kernel
    int roles;                 // workgroups per tile group (LfgcWgradArgs::roles)
    long long dstash_floats, slab_floats_total, dscale_floats, dfeat_floats;
};

Carve carve(const LfgcPlan& p, long long n) {
    Carve c;
    c.nbatches = (n + 255) / 256;                      // whole 256-sample groups, like the forward's stash
    c.ntiles = c.nbatches * 8;
    c.nslabs = (int)(c.ntiles < kMaxSlabs ? c.ntiles : kMaxSlabs);
    if (c.nslabs < 1) c.nslabs = 1;
    // enough tiles: one workgroup per (tile group, layer) instead of per tile group -- the same kMaxSlabs workgroups read
    // the same operands but leave L times fewer slabs (cfg-3 step: 69 -> 17 MB written, and read again by the reduction)
    c.roles = 1;
    if (c.ntiles >= 2LL * kMaxSlabs && p.L > 1 && !getenv("LFGC_WGRAD_NO_SPLIT")) {
        c.roles = p.L;
        c.nslabs = kMaxSlabs / p.L;
    }
    c.dstash_floats = c.ntiles * (long long)p.L * p.stash_layer_floats();
    c.slab_floats_total = (long long)c.nslabs * lfgc_slab_floats(p);
    c.dscale_floats = (c.ntiles * p.L + 3) / 4 * 4;     // one power-of-two scale per (tile, layer), f16 builds
    c.dfeat_floats = c.ntiles * 32 * p.CH;              // feature gradients for the deferred scatter (small batches)
    return c;
}

// The host-side selection of lfgc_backward_f32 for n > 0 samples: lfgc_backward_f32 launches what this returns and
// lfgc_backward_plan reports it.
lfgc_backward_plan_info bwd_select(const LfgcPlan& p, const Carve& c, long long n) {
    lfgc_backward_plan_info b;
    b.CH = p.CH; b.MT = p.MT;
    b.nslabs = c.nslabs; b.roles = c.roles;
    const int cus = lfgc_num_cus();       // per device
    // data kernel: one workgroup per CU, 8 waves once every CU gets a 256-sample batch, else 4 (tiles beyond the
    // last whole 128-sample group are never touched: the stash covers whole 256-sample groups, lfgc_stash_bytes)
    b.waves = ((n + 255) / 256 >= cus) ? 8 : 4;
    b.nbatches = c.nbatches * (8 / b.waves);            // same tile range as the forward wrote
    b.lds_bytes = 4 * lfgc_bwd_lds_floats(p, b.waves);
    b.grid = cus;
    if (b.grid > b.nbatches) b.grid = b.nbatches;
    return b;
}

long long carve_floats(const Carve& c) { return c.dstash_floats + c.slab_floats_total + c.dscale_floats + c.dfeat_floats; }

// lfgc_backward_det_f32's tail behind carve_floats(), 16-byte aligned: int64 accumulator (D,H,W,Cs) | max word (16 bytes)
long long det_offset_bytes(const Carve& c) { return (carve_floats(c) * 4 + 15) / 16 * 16; }
long long det_cells(const LfgcPlan& p, int D, int H, int W) { return (long long)D * H * W * p.CH; }

// What the backward entries and lfgc_input_gradient_f32 share: their checks, in the order each of them makes them
// (`own_null`: one of the entry's own mandatory pointers is null; `own_addrs`: the OR of the entry's own addresses that have
// to be 16-byte aligned), then the plan and every LfgcBwdArgs field that does not depend on the entry.  The rest starts out
// zero: the training build's scratch pointers, stamps, and nbatches (bwd_select's, once an entry knows that n > 0).
int bwd_begin(const lfgc_mlp_desc* desc, const lfgc_positions* positions, const float* grid_cl, int D, int H, int W,
              const float* packed, int precision, const float* stash, const float* d_out, float* d_pos,
              bool own_null, uintptr_t own_addrs, LfgcPlan& p, LfgcBwdArgs& a) {
    if (!desc || !positions || !grid_cl || !packed || !stash || own_null) return LFGC_E_NULL;
    if (!lfgc_mlp_supported(desc)) return LFGC_E_UNSUPPORTED;
    if (!lfgc_precision_supported(precision)) return LFGC_E_UNSUPPORTED;
    if (!positions->pos) return LFGC_E_NULL;            // the backward runs on explicit positions only
    if (positions->n < 0 || D < 1 || H < 1 || W < 1) return LFGC_E_SHAPE;
    if ((((uintptr_t)grid_cl) | ((uintptr_t)packed) | ((uintptr_t)stash) | own_addrs) & 15) return LFGC_E_ALIGN;
    p = lfgc_make_plan(desc->grid_channels, desc->hidden, desc->num_layers, desc->n_freqs);
    a = LfgcBwdArgs{};
    a.pos = positions->pos; a.n = positions->n;
    a.grid = grid_cl; a.D = D; a.H = H; a.W = W; a.Cs = p.CH;
    a.packed = packed; a.L = p.L; a.stash = stash; a.d_out = d_out; a.d_pos = d_pos;
    return LFGC_OK;
}
}  // namespace

extern "C" int lfgc_backward_plan(const lfgc_mlp_desc* desc, int64_t n_samples, int precision, lfgc_backward_plan_info* out) {
    if (!desc || !out) return LFGC_E_NULL;
    if (!lfgc_mlp_supported(desc)) return LFGC_E_UNSUPPORTED;
    if (!lfgc_precision_supported(precision)) return LFGC_E_UNSUPPORTED;
    if (n_samples < 0) return LFGC_E_SHAPE;
    const LfgcPlan p = lfgc_make_plan(desc->grid_channels, desc->hidden, desc->num_layers, desc->n_freqs);
    *out = bwd_select(p, carve(p, n_samples), n_samples);
    return LFGC_OK;
}

extern "C" int64_t lfgc_backward_workspace_bytes(const lfgc_mlp_desc* desc, int64_t n_samples) {
    if (!lfgc_mlp_supported(desc)) return LFGC_E_UNSUPPORTED;
    if (n_samples < 0) return LFGC_E_SHAPE;
    const LfgcPlan p = lfgc_make_plan(desc->grid_channels, desc->hidden, desc->num_layers, desc->n_freqs);
    const Carve c = carve(p, n_samples);
    return carve_floats(c) * 4;
}

extern "C" int64_t lfgc_backward_det_workspace_bytes(const lfgc_mlp_desc* desc, int64_t n_samples, int D, int H, int W) {
    if (!lfgc_mlp_supported(desc)) return LFGC_E_UNSUPPORTED;
    if (n_samples < 0 || D < 1 || H < 1 || W < 1) return LFGC_E_SHAPE;
    const LfgcPlan p = lfgc_make_plan(desc->grid_channels, desc->hidden, desc->num_layers, desc->n_freqs);
    return det_offset_bytes(carve(p, n_samples)) + det_cells(p, D, H, W) * 8 + 16;
}

extern "C" int lfgc_det_quantum_exp(uint32_t max_bits, int64_t n_samples) { return lfgc_det_qexp(max_bits, n_samples); }

// det: lfgc_backward_det_f32 (the deferred feature-gradient path + the fixed-point scatter of lfgc_backward.h)
static int backward_impl(bool det, const lfgc_mlp_desc* desc, const lfgc_positions* positions,
                         const float* grid_cl, int D, int H, int W,
                         const float* packed, int precision, const float* stash, const float* d_out,
                         float* d_grid_cl, float* const* d_weights, float* const* d_biases, float* d_pos,
                         void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    LfgcPlan p;
    LfgcBwdArgs a;
    const int rc0 = bwd_begin(desc, positions, grid_cl, D, H, W, packed, precision, stash, d_out, d_pos,
                              !d_out || !d_grid_cl || !d_weights || !d_biases, ((uintptr_t)d_grid_cl) | ((uintptr_t)workspace), p, a);
    if (rc0 != LFGC_OK) return rc0;
    const long long n = a.n;
    hipStream_t st = (hipStream_t)stream;
    for (int l = 0; l <= p.L; ++l)
        if (!d_weights[l] || !d_biases[l]) return LFGC_E_NULL;
    if (n == 0) {                                       // gradients of an empty batch are zero
        const int K0 = p.E + p.C;
        for (int l = 0; l <= p.L; ++l) {
            const size_t wn = (l == 0) ? (size_t)p.H * K0 : (l == p.L ? (size_t)p.H : (size_t)p.H * p.H);
            const size_t bn = (l == p.L) ? 1 : (size_t)p.H;
            hipError_t e = hipMemsetAsync(d_weights[l], 0, wn * 4, st);
            if (e == hipSuccess) e = hipMemsetAsync(d_biases[l], 0, bn * 4, st);
            if (e != hipSuccess) return (int)e;
        }
        return LFGC_OK;
    }
    const Carve c = carve(p, n);
    const long long cells = det_cells(p, D, H, W);
    const long long need = det ? det_offset_bytes(c) + cells * 8 + 16 : carve_floats(c) * 4;
    if (!workspace || workspace_bytes < need) return LFGC_E_WORKSPACE;
    float* dstash = reinterpret_cast<float*>(workspace);
    float* slabs = dstash + c.dstash_floats;
    float* dscale = slabs + c.slab_floats_total;
    float* dfeat = dscale + c.dscale_floats;

    a.dstash = dstash; a.dscale = dscale; a.d_grid = d_grid_cl;
#ifdef LFGC_STAMPS
    a.stamps = g_bwd_stamps;
#endif

    LfgcWgradArgs w;
    w.stash = stash; w.dstash = dstash; w.d_out = d_out; w.n = n; w.ntiles = c.ntiles; w.L = p.L;
    w.slabs = slabs; w.slab_floats = lfgc_slab_floats(p);
    w.dscale = precision == LFGC_PRECISION_F32 ? nullptr : dscale;     // f16 builds: f16-split contraction (lfgc_bwd_weight.h)

    const lfgc_backward_plan_info b = bwd_select(p, c, n);
    w.roles = b.roles;
    // Feature-gradient scatter: inside the data kernel.  LFGC_SCATTER=deferred (diagnostics) moves the float atomics into
    // a kernel of their own at full occupancy: measured at the cfg-3 train step, the data kernel drops from 78 to 54 us and
    // the scatter kernel takes 29 us -- 8.4 M device-scope float adds on cold lines cost that much either way (the
    // in-kernel phase stamps' 40 % "scatter" share is their latency, not an occupancy problem), so the step does not move.
    {
        const char* env = getenv("LFGC_SCATTER");
        a.dfeat = (det || (env && env[0] == 'd')) ? dfeat : nullptr;
    }
    a.nbatches = b.nbatches;
    LfgcDetScatter ds;
    ds.acc = reinterpret_cast<long long*>(reinterpret_cast<char*>(workspace) + det_offset_bytes(c));
    ds.maxw = reinterpret_cast<unsigned*>(ds.acc + cells);
    if (det) {
        if ((cells / 2 + 255) / 256 > 0x7fffffffLL) return LFGC_E_UNSUPPORTED;
        hipLaunchKernelGGL(lfgc_det_zero_kernel, dim3((unsigned)((cells / 2 + 255) / 256)), dim3(256), 0, st, ds.acc, cells, ds.maxw);
        LFGC_HIP_CHECK_LAUNCH();
    }

    const int rc = kBwd[p.CH / 8 - 1](p.MT, a, w, b.waves, precision, b.lds_bytes, (int)b.grid, b.nslabs * b.roles, st,
                                      det ? &ds : nullptr);
    if (rc != LFGC_OK) return rc;
    if (det) {
        hipLaunchKernelGGL(lfgc_det_finish_kernel, dim3((unsigned)((cells / 4 + 255) / 256)), dim3(256), 0, st, ds.acc, ds.maxw, n,
                           d_grid_cl, cells);
        LFGC_HIP_CHECK_LAUNCH();
    }

    LfgcReduceArgs r;
    r.slabs = slabs; r.nslabs = b.nslabs; r.slab_floats = w.slab_floats; r.plan = p;
    for (int l = 0; l <= p.L; ++l) { r.dw[l] = d_weights[l]; r.db[l] = d_biases[l]; }
    for (int i = 0; i < 64; ++i) r.col_of_src[i] = 0;
    for (int cl = 0; cl < p.K0P; ++cl) {
        const int src = lfgc_layer0_src_col(p, cl);
        if (src >= 0) r.col_of_src[src] = cl;
    }
    const int K0 = p.E + p.C;
    const int total = p.H * K0 + p.H + (p.L - 1) * (p.H * p.H + p.H) + p.H + 1;
    const int g = (total + 63) / 64;
    hipLaunchKernelGGL(lfgc_bwd_reduce_kernel, dim3(g), dim3(256), 0, st, r);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_backward_f32(const lfgc_mlp_desc* desc, const lfgc_positions* positions,
                                 const float* grid_cl, int D, int H, int W,
                                 const float* packed, int precision, const float* stash, const float* d_out,
                                 float* d_grid_cl, float* const* d_weights, float* const* d_biases, float* d_pos,
                                 void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    return backward_impl(false, desc, positions, grid_cl, D, H, W, packed, precision, stash, d_out, d_grid_cl, d_weights, d_biases,
                         d_pos, workspace, workspace_bytes, stream);
}

extern "C" int lfgc_backward_det_f32(const lfgc_mlp_desc* desc, const lfgc_positions* positions,
                                     const float* grid_cl, int D, int H, int W,
                                     const float* packed, int precision, const float* stash, const float* d_out,
                                     float* d_grid_cl, float* const* d_weights, float* const* d_biases, float* d_pos,
                                     void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    return backward_impl(true, desc, positions, grid_cl, D, H, W, packed, precision, stash, d_out, d_grid_cl, d_weights, d_biases,
                         d_pos, workspace, workspace_bytes, stream);
}

// The input-gradient entry: the data kernel's INPUT_ONLY build under the launch bwd_select picks for the training build
// (the same carve, waves, passes and grid), and nothing else -- no workspace, no weight-gradient kernel, no reduction.
extern "C" int lfgc_input_gradient_plan(const lfgc_mlp_desc* desc, int64_t n_samples, int precision, lfgc_backward_plan_info* out) {
    const int rc = lfgc_backward_plan(desc, n_samples, precision, out);
    if (rc == LFGC_OK) out->nslabs = out->roles = 0;      // there is no weight-gradient kernel behind this one
    return rc;
}

extern "C" int lfgc_input_gradient_f32(const lfgc_mlp_desc* desc, const lfgc_positions* positions,
                                       const float* grid_cl, int D, int H, int W,
                                       const float* packed, int precision, const float* stash, const float* d_out,
                                       float* d_pos, lfgc_stream_t stream) {
    LfgcPlan p;
    LfgcBwdArgs a;
    const int rc = bwd_begin(desc, positions, grid_cl, D, H, W, packed, precision, stash, d_out, d_pos, !d_pos, 0, p, a);
    if (rc != LFGC_OK) return rc;
    if (a.n == 0) return LFGC_OK;
    const lfgc_backward_plan_info b = bwd_select(p, carve(p, a.n), a.n);
    a.nbatches = b.nbatches;
    return kIgrad[p.CH / 8 - 1](p.MT, a, b.waves, precision, b.lds_bytes, (int)b.grid, (hipStream_t)stream);
}

extern "C" int lfgc_backward_bf16(const lfgc_mlp_desc* desc, const lfgc_positions* positions, const float* grid_cl, int D, int H,
                                  int W, const float* packed, const float* stash, const float* d_out, float* d_grid_cl,
                                  float* const* d_weights, float* const* d_biases, float* d_pos,
                                  void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    return lfgc_backward_f32(desc, positions, grid_cl, D, H, W, packed, LFGC_PRECISION_F16, stash, d_out, d_grid_cl, d_weights,
                             d_biases, d_pos, workspace, workspace_bytes, stream);
}
