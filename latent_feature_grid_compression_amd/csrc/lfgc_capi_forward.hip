// lfgc_capi_forward.hip -- C-ABI entry for the fused forward: argument checks, plan, dispatch.
#include <stdlib.h>
#include "lfgc_forward16.h"      // the LDS layouts of both kernel families (lfgc_fwd_lds_floats, lfgc_fwd16_lds_floats)

typedef int LfgcFwdDispatch(int MT, const LfgcFwdArgs& a, int lds_bytes, int grid, hipStream_t stream);
LfgcFwdDispatch lfgc_fwd_dispatch_ch8, lfgc_fwd_dispatch_ch16, lfgc_fwd_dispatch_ch24, lfgc_fwd_dispatch_ch32;
LfgcFwdDispatch lfgc_fwd16_dispatch_ch8, lfgc_fwd16_dispatch_ch16, lfgc_fwd16_dispatch_ch24, lfgc_fwd16_dispatch_ch32;

namespace {
// The per-channel instantiation files' entries, by CH / 8 - 1 (CH = 8, 16, 24, 32: lfgc_mlp_supported).
LfgcFwdDispatch* const kFwd[4] = {lfgc_fwd_dispatch_ch8, lfgc_fwd_dispatch_ch16, lfgc_fwd_dispatch_ch24, lfgc_fwd_dispatch_ch32};
LfgcFwdDispatch* const kFwd16[4] = {lfgc_fwd16_dispatch_ch8, lfgc_fwd16_dispatch_ch16, lfgc_fwd16_dispatch_ch24, lfgc_fwd16_dispatch_ch32};
int num_cus() { return lfgc_num_cus(); }
#ifdef LFGC_STAMPS
unsigned long long* g_stamps = nullptr;
#endif
}  // namespace

__global__ void lfgc_clear_word_kernel(int32_t* w) {
    if (threadIdx.x == 0) __hip_atomic_store(w, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#ifdef LFGC_STAMPS
// Diagnostics builds only (tools/phase_stamps.py): device buffer of 16 counters per wave slot (grid x 8 waves).
extern "C" void lfgc_debug_set_stamp_buffer(void* p) { g_stamps = reinterpret_cast<unsigned long long*>(p); }
#endif

// Validates `positions` and fills the position part of the kernel arguments; returns the sample count
// through *n_out.
int lfgc_fill_positions(const lfgc_positions* ps, LfgcFwdArgs* a, long long* n_out) {
    if (!ps) return LFGC_E_NULL;
    if (ps->pos) {
        if (ps->n < 0) return LFGC_E_SHAPE;
        a->pos = ps->pos;
        *n_out = ps->n;
        a->res0 = a->res1 = a->res2 = 2; a->x_begin = 0; a->tile = 32;
        a->scale0 = a->scale1 = a->scale2 = 1.0f;
        return LFGC_OK;
    }
    if (ps->res[0] < 2 || ps->res[1] < 2 || ps->res[2] < 2 || ps->tile < 1) return LFGC_E_SHAPE;
    if (ps->x_begin < 0 || ps->x_end > ps->res[0] || ps->x_end < ps->x_begin) return LFGC_E_SHAPE;
    a->pos = nullptr;
    a->res0 = ps->res[0]; a->res1 = ps->res[1]; a->res2 = ps->res[2];
    a->x_begin = ps->x_begin; a->tile = ps->tile;
    // dataset.scales = max_idx / max(max_idx)     (data/IndexDataset.py:64-65), fp32 division
    const float m0 = (float)(ps->res[0] - 1), m1 = (float)(ps->res[1] - 1), m2 = (float)(ps->res[2] - 1);
    const float mm = m0 > m1 ? (m0 > m2 ? m0 : m2) : (m1 > m2 ? m1 : m2);
    a->scale0 = m0 / mm; a->scale1 = m1 / mm; a->scale2 = m2 / mm;
    *n_out = (long long)(ps->x_end - ps->x_begin) * ps->res[1] * ps->res[2];
    return LFGC_OK;
}

namespace {
// Shape checks the launch and the plan query share (everything lfgc_forward_f32 refuses that is not a pointer).
int fwd_check_shape(const lfgc_mlp_desc* desc, int D, int H, int W, int precision) {
    if (!lfgc_mlp_supported(desc)) return LFGC_E_UNSUPPORTED;
    if (D < 1 || H < 1 || W < 1) return LFGC_E_SHAPE;
    if ((long long)D * H * W * lfgc_roundup(desc->grid_channels, 8) >= (1LL << 30)) return LFGC_E_UNSUPPORTED;   // 32-bit byte offsets
    if (!lfgc_precision_supported(precision)) return LFGC_E_UNSUPPORTED;
    return LFGC_OK;
}

int fwd_env_waves(int resident, int waves) {            // diagnostics: LFGC_FWD_WAVES=4|8, streamed nets only
    if (const char* e = getenv("LFGC_FWD_WAVES")) { if (!resident && (e[0] == '4' || e[0] == '8')) return e[0] - '0'; }
    return waves;
}
// diagnostics: LFGC_FWD_RUNTIME_DEPTH=1 runs the any-depth f16 kernels on 4-layer nets too -- the baseline arm of same-tree
// A/Bs (tools/ab_forward.py) and the reference of tests/test_fwd_static_depth_gpu.py
int fwd_env_runtime_depth() {
    const char* e = getenv("LFGC_FWD_RUNTIME_DEPTH");
    return (e && e[0] == '1') ? 1 : 0;
}

long long fwd_lds_bytes(const LfgcPlan& p, bool h16, bool resident, long long table_floats, int nzc) {
    return 4 * (h16 ? lfgc_fwd16_lds_floats(p, resident, table_floats, nzc) : lfgc_fwd_lds_floats(p, resident, table_floats));
}
long long fwd_table_floats(const LfgcFwdArgs& a) { return (long long)a.res0 + a.res1 + a.res2; }
int fwd_lds_cap(int resident) { return resident ? LFGC_LDS_BYTES_RESIDENT : LFGC_LDS_BYTES_STREAMED; }

// One launch of the exact-fp32 build (h16 = false) or of an f16 build before its z-run decision (h16 = true).
lfgc_forward_launch fwd_base_launch(const LfgcPlan& p, const LfgcFwdArgs& a, long long n, bool h16, bool env_waves) {
    lfgc_forward_launch l;
    // LDS as the kernels carve it (lfgc_fwd_lds_floats, lfgc_fwd16_lds_floats): every layer block when that fits
    // (resident: 4-wave workgroups, two per CU), else a 2-deep ring of the largest block (streamed: 8-wave workgroups, one per
    // CU).  The stash is laid out per 32-sample tile in whole 128-sample groups either way (lfgc_stash_bytes), so both
    // builds write the same format.
    l.resident = fwd_lds_bytes(p, h16, true, 0, 0) <= LFGC_LDS_BYTES_RESIDENT ? 1 : 0;
    l.lds_bytes = (int)fwd_lds_bytes(p, h16, l.resident, 0, 0);
    l.coord_table = 0;
    if (!a.pos) {                                       // per-axis coordinate tables behind the weight region, if they fit
        const long long with_tables = fwd_lds_bytes(p, h16, l.resident, fwd_table_floats(a), 0);
        if (with_tables <= fwd_lds_cap(l.resident)) { l.coord_table = 1; l.lds_bytes = (int)with_tables; }
    }
    // streamed nets: 8-wave workgroups once every CU gets at least one 256-sample batch, else 4-wave ones
    l.waves = (!l.resident && (n + 255) / 256 >= num_cus()) ? 8 : 4;
    if (env_waves) l.waves = fwd_env_waves(l.resident, l.waves);
    // always whole 256-sample groups of tiles, so the stash covers the same tile range whichever build runs
    l.nbatches = (n + 255) / 256 * (8 / l.waves);
    l.zrun = 0; l.nzc = 2; l.tiles_per_row = 1; l.ntiles = 0; l.x2 = 0;
    l.grid = 0;
    return l;
}

void fwd_set_grid(lfgc_forward_launch* l) {
    l->grid = (l->resident ? 2LL : 1LL) * num_cus();
    if (l->grid > l->nbatches) l->grid = l->nbatches;
}

// The host-side selection of lfgc_forward_f32: fills the position part of *a (lfgc_fill_positions), *n and *out.
// lfgc_forward_f32 launches what *out says and lfgc_forward_plan reports it.
int fwd_select(const lfgc_mlp_desc* desc, const lfgc_positions* positions, int D, int precision, bool has_stash,
               bool has_status, const LfgcPlan& p, LfgcFwdArgs* a, long long* n_out, lfgc_forward_plan_info* out) {
    long long n = 0;
    const int rc = lfgc_fill_positions(positions, a, &n);
    if (rc != LFGC_OK) return rc;
    *n_out = n;
    const bool h16 = precision != LFGC_PRECISION_F32;
    out->CH = p.CH; out->MT = p.MT; out->reserved = 0;
    out->has_redo = (h16 && has_status) ? 1 : 0;
    lfgc_forward_launch l = fwd_base_launch(p, *a, n, h16, true);
    // Lattice mode on the f16 builds: z-run tiles + column sampler (lfgc_forward.h) when the column a 32-voxel run touches
    // is short (volume at least ~3x finer than the grid along z: every BASELINE full-volume shape) and fits the LDS left.
    if (h16 && !a->pos && l.coord_table && !has_stash && !getenv("LFGC_NO_ZRUN")) {
        const int nzc = (int)(31.0 * (double)D / (double)(a->res2 - 1) + 1e-3) + 3;
        const long long rows = (long long)(positions->x_end - positions->x_begin) * a->res1;
        const int tpr = (a->res2 + LFGC_TILE_SAMPLES - 1) / LFGC_TILE_SAMPLES;
        const long long ntiles = rows * tpr;
        const long long with_columns = fwd_lds_bytes(p, true, l.resident, fwd_table_floats(*a), nzc);
        if (nzc <= LFGC_NZC_MAX && ntiles < (1LL << 31) && with_columns <= fwd_lds_cap(l.resident)) {
            l.zrun = 1; l.nzc = nzc; l.tiles_per_row = tpr; l.ntiles = ntiles;
            l.lds_bytes = (int)with_columns;
            l.waves = fwd_env_waves(l.resident, (!l.resident && (ntiles + 7) / 8 >= num_cus()) ? 8 : 4);
            l.nbatches = (ntiles + l.waves - 1) / l.waves;
        }
    }
    fwd_set_grid(&l);
    out->first = l;
    if (out->has_redo) {
        // Range fallback: the same pass on the exact-fp32 build; residency, workgroup shape and grid are its own.
        out->redo = fwd_base_launch(p, *a, n, false, false);
        fwd_set_grid(&out->redo);
    } else {
        out->redo = lfgc_forward_launch{};
    }
    return LFGC_OK;
}

void fwd_apply_launch(const lfgc_forward_launch& l, LfgcFwdArgs* a) {
    a->resident = l.resident; a->waves = l.waves; a->coord_table = l.coord_table; a->nbatches = l.nbatches;
    a->zrun = l.zrun; a->nzc = l.nzc; a->tiles_per_row = l.tiles_per_row; a->ntiles = l.ntiles;
}
}  // namespace

extern "C" int lfgc_forward_plan(const lfgc_mlp_desc* desc, const lfgc_positions* positions, int D, int H, int W, int precision,
                                 int has_stash, int has_status, lfgc_forward_plan_info* out) {
    if (!desc || !positions || !out) return LFGC_E_NULL;
    const int rc = fwd_check_shape(desc, D, H, W, precision);
    if (rc != LFGC_OK) return rc;
    const LfgcPlan p = lfgc_make_plan(desc->grid_channels, desc->hidden, desc->num_layers, desc->n_freqs);
    LfgcFwdArgs a;
    long long n = 0;
    return fwd_select(desc, positions, D, precision, has_stash != 0, has_status != 0, p, &a, &n, out);
}

extern "C" int lfgc_forward_f32(const lfgc_mlp_desc* desc, const lfgc_positions* positions,
                                const float* grid_cl, int D, int H, int W,
                                const float* packed, int precision, int clamp, float* out, float* stash,
                                int32_t* status, lfgc_stream_t stream) {
    if (!desc || !positions || !grid_cl || !packed || !out) return LFGC_E_NULL;
    const int rcs = fwd_check_shape(desc, D, H, W, precision);
    if (rcs != LFGC_OK) return rcs;
    if ((((uintptr_t)grid_cl) | ((uintptr_t)packed)) & 15) return LFGC_E_ALIGN;
    const LfgcPlan p = lfgc_make_plan(desc->grid_channels, desc->hidden, desc->num_layers, desc->n_freqs);
    LfgcFwdArgs a;
    long long n = 0;
    lfgc_forward_plan_info plan;
    const int rc = fwd_select(desc, positions, D, precision, stash != nullptr, status != nullptr, p, &a, &n, &plan);
    if (rc != LFGC_OK) return rc;
    if (n == 0) return LFGC_OK;
    a.n = n;
    a.grid = grid_cl; a.D = D; a.H = H; a.W = W; a.Cs = p.CH;
    a.packed = packed; a.L = p.L; a.clamp = clamp; a.out = out; a.stash = stash;
    const bool h16 = precision != LFGC_PRECISION_F32;
    a.single = precision == LFGC_PRECISION_F16 ? 1 : 0;
    a.status = nullptr; a.redo_if = nullptr; a.stamps = nullptr;
    a.runtime_depth = fwd_env_runtime_depth();
#ifdef LFGC_STAMPS
    a.stamps = g_stamps;
#endif
    fwd_apply_launch(plan.first, &a);
    hipStream_t st = (hipStream_t)stream;
    if (h16) {
        if (status) {
            // range screen on: cleared here, set by the kernel, read by the predicated redo -- all in stream order.
            // Cleared by a kernel of our own, NOT hipMemsetAsync: inside a captured HIP graph (ROCm 7.2) the memset
            // node of a 4-byte clear did not take effect before the following kernel nodes on replay -- the redo then
            // ran in full on every replay of a captured train step (measured: 58 us instead of 4 us; profiles/r2).
            hipLaunchKernelGGL(lfgc_clear_word_kernel, dim3(1), dim3(64), 0, st, status);
            LFGC_HIP_CHECK_LAUNCH();
            a.status = status;
        }
        const int rc16 = kFwd16[p.CH / 8 - 1](p.MT, a, plan.first.lds_bytes, (int)plan.first.grid, st);
        if (rc16 != LFGC_OK || !plan.has_redo) return rc16;
        // Range fallback: the same pass on the exact-fp32 build, enqueued behind the fast one; its workgroups return
        // at once unless the fast kernel has set *status (a sample left the f16 range: diverged or very wide model).
        // No host synchronisation, graph-capturable; costs one empty launch when nothing overflowed.
        a.status = nullptr; a.redo_if = status; a.single = 0;
        fwd_apply_launch(plan.redo, &a);
    }
    const lfgc_forward_launch& l32 = h16 ? plan.redo : plan.first;
    return kFwd[p.CH / 8 - 1](p.MT, a, l32.lds_bytes, (int)l32.grid, st);
}

extern "C" int lfgc_forward_bf16(const lfgc_mlp_desc* desc, const lfgc_positions* positions, const float* grid_cl, int D, int H,
                                 int W, const float* packed, int clamp, float* out, float* stash, int32_t* status,
                                 lfgc_stream_t stream) {
    return lfgc_forward_f32(desc, positions, grid_cl, D, H, W, packed, LFGC_PRECISION_F16, clamp, out, stash, status, stream);
}
