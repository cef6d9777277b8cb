// lfgc_backward.hip -- C-ABI entry for the backward of the fused path: checks, workspace carving, dispatch.
#include <cstdlib>
#include "lfgc_backward.h"

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
}  // namespace

extern "C" int lfgc_backward_plan(const lfgc_mlp_desc* desc, int64_t n_samples, int precision, lfgc_backward_plan_info* out) {
    if (!desc || !out) return LFGC_E_NULL;
    if (!lfgc_mlp_supported(desc)) return LFGC_E_UNSUPPORTED;
    if (precision != LFGC_PRECISION_F32 && precision != LFGC_PRECISION_F16X2 && precision != LFGC_PRECISION_F16) return LFGC_E_UNSUPPORTED;
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
    if (!desc || !positions || !grid_cl || !packed || !stash || !d_out || !d_grid_cl || !d_weights || !d_biases)
        return LFGC_E_NULL;
    if (!lfgc_mlp_supported(desc)) return LFGC_E_UNSUPPORTED;
    if (precision != LFGC_PRECISION_F32 && precision != LFGC_PRECISION_F16X2 && precision != LFGC_PRECISION_F16) return LFGC_E_UNSUPPORTED;
    if (!positions->pos) return LFGC_E_NULL;            // backward runs on explicit positions only
    if (positions->n < 0 || D < 1 || H < 1 || W < 1) return LFGC_E_SHAPE;
    if ((((uintptr_t)grid_cl) | ((uintptr_t)packed) | ((uintptr_t)stash) | ((uintptr_t)d_grid_cl) | ((uintptr_t)workspace)) & 15)
        return LFGC_E_ALIGN;
    const LfgcPlan p = lfgc_make_plan(desc->grid_channels, desc->hidden, desc->num_layers, desc->n_freqs);
    const long long n = positions->n;
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

    LfgcBwdArgs a;
    a.pos = positions->pos; a.n = n;
    a.grid = grid_cl; a.D = D; a.H = H; a.W = W; a.Cs = p.CH;
    a.packed = packed; a.L = p.L; a.stash = stash; a.d_out = d_out;
    a.dstash = dstash; a.dscale = dscale; a.d_grid = d_grid_cl; a.d_pos = d_pos;
    a.stamps = nullptr;
#ifdef LFGC_STAMPS
    a.stamps = g_bwd_stamps;
#endif

    LfgcWgradArgs w;
    w.stash = stash; w.dstash = dstash; w.d_out = d_out; w.n = n; w.ntiles = c.ntiles; w.L = p.L;
    w.slabs = slabs; w.slab_floats = lfgc_slab_floats(p);
    w.dscale = precision == LFGC_PRECISION_F32 ? nullptr : dscale;     // f16 builds: f16-split contraction (lfgc_backward.h)

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
    if (!desc || !positions || !grid_cl || !packed || !stash || !d_pos) return LFGC_E_NULL;
    if (!lfgc_mlp_supported(desc)) return LFGC_E_UNSUPPORTED;
    if (precision != LFGC_PRECISION_F32 && precision != LFGC_PRECISION_F16X2 && precision != LFGC_PRECISION_F16) return LFGC_E_UNSUPPORTED;
    if (!positions->pos) return LFGC_E_NULL;            // explicit positions only, like the backward
    if (positions->n < 0 || D < 1 || H < 1 || W < 1) return LFGC_E_SHAPE;
    if ((((uintptr_t)grid_cl) | ((uintptr_t)packed) | ((uintptr_t)stash)) & 15) return LFGC_E_ALIGN;
    const long long n = positions->n;
    if (n == 0) return LFGC_OK;
    const LfgcPlan p = lfgc_make_plan(desc->grid_channels, desc->hidden, desc->num_layers, desc->n_freqs);
    const lfgc_backward_plan_info b = bwd_select(p, carve(p, n), n);

    LfgcBwdArgs a;
    a.pos = positions->pos; a.n = n;
    a.grid = grid_cl; a.D = D; a.H = H; a.W = W; a.Cs = p.CH;
    a.packed = packed; a.L = p.L; a.stash = stash; a.d_out = d_out;
    a.dstash = nullptr; a.dscale = nullptr; a.d_grid = nullptr; a.dfeat = nullptr; a.d_pos = d_pos;
    a.nbatches = b.nbatches;
    a.stamps = nullptr;
    return kIgrad[p.CH / 8 - 1](p.MT, a, b.waves, precision, b.lds_bytes, (int)b.grid, (hipStream_t)stream);
}

extern "C" int lfgc_backward_bf16(const lfgc_mlp_desc* desc, const lfgc_positions* positions, const float* grid_cl, int D, int H,
                                  int W, const float* packed, const float* stash, const float* d_out, float* d_grid_cl,
                                  float* const* d_weights, float* const* d_biases, float* d_pos,
                                  void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    return lfgc_backward_f32(desc, positions, grid_cl, D, H, W, packed, LFGC_PRECISION_F16, stash, d_out, d_grid_cl, d_weights,
                             d_biases, d_pos, workspace, workspace_bytes, stream);
}
