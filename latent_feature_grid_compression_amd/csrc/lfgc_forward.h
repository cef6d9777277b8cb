// lfgc_forward.h -- fused trilinear sample + Fourier embed + SnakeAlt MLP forward for gfx950.
//
// Replaces model/Feature_Grid_Model.py:62-78 of the reference (grid_sample, Embedder.embed, cat,
// L x (Linear + SnakeAlt), final Linear, optional clamp).
//
// Mapping (one wave = 32 samples, v_mfma_f32_32x32x2_f32, exact fp32):
//   Out^T[h_out, sample] = W[h_out, k] . In^T[k, sample]
//   A operand = W tile from LDS      lane (i = lane&31, hh = lane>>5) supplies W[32m + i][k(s, hh)]
//   B operand = activations in VGPRs lane (j = lane&31, hh)           supplies In[k(s, hh)][sample j]
//   C/D       = 16 accumulators      lane (j, hh), reg r = row 32m + (r&3) + 8(r>>2) + 4hh of sample j
// The k order is chosen as k(s, hh) = 32(s>>4) + 8((s>>2)&3) + 4hh + (s&3), which is exactly the row a
// lane's accumulator register r = s&15 of tile m = s>>4 holds: after SnakeAlt the accumulators ARE the
// next layer's B operands, so activations never leave registers and never cross lanes.  With that
// order a lane's A values for 4 consecutive k-steps are 4 consecutive floats of one W row: one
// ds_read_b128 feeds 4 MFMAs.
// Nets whose layer blocks all fit 80 KB of LDS: workgroup = 4 waves = 128 samples, blocks staged once, two
// workgroups per CU.  Larger nets: workgroup = 8 waves = 256 samples, one per CU, layer blocks stream through a
// 2-deep LDS ring by LDS-DMA (next layer in flight while the current one computes, one barrier per layer).
#pragma once
#include "lfgc_common.h"

// Diagnostics only (tools/ablate_forward.py builds separate libraries with -DLFGC_ABLATE=mask; the shipped
// library is always built with 0): 1 = no gather loads, 2 = activation replaced by 0.5*a, 4 = no MFMAs.
#ifndef LFGC_ABLATE
#define LFGC_ABLATE 0
#endif

struct LfgcFwdArgs {
    const float* pos;          // (N,3) or nullptr (lattice mode)
    long long n;               // samples
    int res0, res1, res2;      // lattice mode: volume resolution
    int x_begin;               // lattice mode: first x of the slab
    int tile;                  // lattice mode: tile edge (32)
    float scale0, scale1, scale2;   // lattice mode: dataset.scales (data/IndexDataset.py:64-65)
    const float* grid;         // (D,H,W,Cs)
    int D, H, W, Cs;
    const float* packed;
    int L;
    int resident;              // 1: all layer blocks staged once
    int clamp;
    float* out;                // (N)
    float* stash;              // or nullptr
    long long nbatches;        // ceil(N / (32 * waves per workgroup))
    int waves;                 // waves per workgroup of the chosen build (4 or 8)
    int coord_table;           // lattice mode: per-axis coordinate tables fit LDS (res0+res1+res2 floats)
    int single;                // f16 builds: 1 = single product W_hi.h_hi (LFGC_PRECISION_F16), 0 = hi/lo split
    int* status;               // f16 builds: set to 1 when a sample left the range of the fast arithmetic (or nullptr)
    const int* redo_if;        // exact build: run only if *redo_if != 0 (nullptr: always) -- the range fallback
    unsigned long long* stamps;   // diagnostics builds (-DLFGC_STAMPS, tools/phase_stamps.py): per-wave cycle totals per phase
    // lattice mode, f16 builds: "z-run" tiles (LfgcColumnSampler): a wave's 32 samples are 32 consecutive z of ONE (x, y)
    // row of the slab; tiles_per_row = ceil(res2 / 32), ntiles = rows * tiles_per_row, nzc = z cells a tile's column holds
    int zrun, nzc, tiles_per_row;
    // f16 builds, read by the launcher only: 1 = the any-depth kernel even where a depth-specialised one exists
    // (diagnostics: LFGC_FWD_RUNTIME_DEPTH).  It sits in what was padding before `ntiles`: no other member moves.
    int runtime_depth;
    long long ntiles;
};
static_assert(sizeof(LfgcFwdArgs) == 184 && offsetof(LfgcFwdArgs, ntiles) == 176, "kernel-argument layout");

// Lattice coordinate of voxel v along one axis, formed like field_from_net does per tile
// (visualization/OutputToVTK.py:23-37) + torch.linspace's CPU formula (start + step*i below the
// midpoint, end - step*(n-1-i) above).  ATen's build contracts each of the two into ONE fused multiply-add on every host
// with FMA units (ATEN_CPU_CAPABILITY avx2 / avx512; only the `default` capability rounds the product first), and the
// reference's recorded tiles (tests/golden/tiles_70x40x33.npz) carry that rounding: so does this function.  The unfused
// form was off by one ulp of the linspace value (1.2e-7 after 2x - 1) at about a tenth of the coordinates of a lattice
// whose edge - 1 is no power of two; a 256-voxel edge gives the same bits either way.
__device__ __forceinline__ float lfgc_lattice_coord(int v, int res, int tile, float scale) {
    const int tb = (v / tile) * tile;
    const int te = min(tb + tile, res);
    const int cnt = te - tb;
    const int i = v - tb;
    const float max_idx = (float)(res - 1);
    const float min_alpha = (float)((double)tb / (double)(res - 1));
    const float max_alpha = (float)((double)(te - 1) / (double)(res - 1));
    const float min_bounds = __fadd_rn(0.0f, __fmul_rn(min_alpha, max_idx));
    const float max_bounds = __fadd_rn(0.0f, __fmul_rn(max_alpha, max_idx));
    const float start = __fdiv_rn(min_bounds, max_idx);
    const float end = __fdiv_rn(max_bounds, max_idx);
    float lin;
    if (cnt == 1) {
        lin = start;
    } else {
        const float step = __fdiv_rn(__fsub_rn(end, start), (float)(cnt - 1));
        lin = (i < cnt / 2) ? __fmaf_rn(step, (float)i, start)
                            : __fmaf_rn(-step, (float)(cnt - i - 1), end);
    }
    const float nrm = __fsub_rn(__fmul_rn(2.0f, lin), 1.0f);
    return __fmul_rn(scale, nrm);
}

// Lattice mode: the coordinate of every voxel index, axis after axis (res0 | res1 | res2 floats), built once per workgroup
// of nt threads; the caller's barrier publishes it.
__device__ __forceinline__ void lfgc_fill_coord_table(const LfgcFwdArgs& a, float* s_coord, int tid, int nt) {
    const int r01 = a.res0 + a.res1, r012 = r01 + a.res2;
    for (int i = tid; i < r012; i += nt) {
        s_coord[i] = i < a.res0 ? lfgc_lattice_coord(i, a.res0, a.tile, a.scale0)
                   : i < r01 ? lfgc_lattice_coord(i - a.res0, a.res1, a.tile, a.scale1)
                             : lfgc_lattice_coord(i - r01, a.res2, a.tile, a.scale2);
    }
}

// sk[k][ax] = sin(f_k p_ax), ck[k][ax] = cos(f_k p_ax): the argument is one fp32 product, the fast evaluation is redone
// on the slow path by the whole wave when any lane's argument leaves its range.  Shared by the forward's embedding
// (generic NF) and the backward's d_pos.
template <int NF>
__device__ __forceinline__ void lfgc_fourier_trig(float p0, float p1, float p2, float (&sk)[NF > 0 ? NF : 1][3],
                                                  float (&ck)[NF > 0 ? NF : 1][3]) {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const float f = lfgc_freq(k);
        const float a0 = __fmul_rn(p0, f), a1 = __fmul_rn(p1, f), a2 = __fmul_rn(p2, f);
        bad |= lfgc_trig_out_of_range(a0) | lfgc_trig_out_of_range(a1) | lfgc_trig_out_of_range(a2);
        lfgc_sincosf_t<false>(a0, sk[k][0], ck[k][0]);
        lfgc_sincosf_t<false>(a1, sk[k][1], ck[k][1]);
        lfgc_sincosf_t<false>(a2, sk[k][2], ck[k][2]);
    }
    if (__builtin_expect(__any(bad), 0)) {   // positions far outside [-1,1], inf or nan
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            const float f = lfgc_freq(k);
            lfgc_sincosf_t<true>(__fmul_rn(p0, f), sk[k][0], ck[k][0]);
            lfgc_sincosf_t<true>(__fmul_rn(p1, f), sk[k][1], ck[k][1]);
            lfgc_sincosf_t<true>(__fmul_rn(p2, f), sk[k][2], ck[k][2]);
        }
    }
}

// Scalar inputs [p | sin f_k p | cos f_k p | 0 pad] of the lane's sample: a lane keeps only its half of the list
// (E[0 .. EP/2) = entries [hh EP/2, (hh+1) EP/2)).
template <int NF>
__device__ __forceinline__ void lfgc_embed_inputs(float p0, float p1, float p2, int hh, float* __restrict__ E) {
    constexpr LfgcPlan P = LfgcShape<8, 1, NF>::P;      // the scalar inputs depend on NF alone
    constexpr int EP = P.EP, EPH = P.EPH(), E_ = P.E;

        // ---- scalar inputs [p | sin f_k p | cos f_k p]: a lane keeps only its half of the list ---------------------
        if constexpr (NF == 2) {
            // e = [p0 p1 p2 s0x s0y s0z c0x c0y | c0z s1x s1y s1z c1x c1y c1z 0] (f0, f1 = 2 f0): lane half 0 needs sin/cos
            // of f0 p, lane half 1 those of f1 p plus cos(f0 p2) -- three sincos of lane-half-dependent arguments and one
            // cosine instead of six sincos per lane.  Arguments are formed as before (one fp32 product each).
            const float f0 = lfgc_freq(0), f1 = lfgc_freq(1);
            const float f = hh ? f1 : f0;
            const float a0 = __fmul_rn(p0, f), a1 = __fmul_rn(p1, f), a2 = __fmul_rn(p2, f), a3 = __fmul_rn(p2, f0);
            const bool bad = lfgc_trig_out_of_range(a0) | lfgc_trig_out_of_range(a1) | lfgc_trig_out_of_range(a2) |
                             lfgc_trig_out_of_range(a3);
            float sA, cA, sB, cB, sC, cC, sD, cD;
            lfgc_sincosf_t<false>(a0, sA, cA);
            lfgc_sincosf_t<false>(a1, sB, cB);
            lfgc_sincosf_t<false>(a2, sC, cC);
            cD = lfgc_cosf_t<false>(a3);
            if (__builtin_expect(__any(bad), 0)) {   // positions far outside [-1,1], inf or nan
                lfgc_sincosf_t<true>(a0, sA, cA);
                lfgc_sincosf_t<true>(a1, sB, cB);
                lfgc_sincosf_t<true>(a2, sC, cC);
                lfgc_sincosf_t<true>(a3, sD, cD);
            }
            const float lo[8] = {p0, p1, p2, sA, sB, sC, cA, cB};
            const float hi[8] = {cD, sA, sB, sC, cA, cB, cC, 0.0f};
#pragma unroll
            for (int t = 0; t < EPH; ++t) E[t] = hh ? hi[t] : lo[t];
        } else {
            float e[EP], sk[NF > 0 ? NF : 1][3], ck[NF > 0 ? NF : 1][3];
            e[0] = p0; e[1] = p1; e[2] = p2;
            lfgc_fourier_trig<NF>(p0, p1, p2, sk, ck);
#pragma unroll
            for (int k = 0; k < NF; ++k) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) { e[3 + 6 * k + ax] = sk[k][ax]; e[3 + 6 * k + 3 + ax] = ck[k][ax]; }
            }
#pragma unroll
            for (int t = E_; t < EP; ++t) e[t] = 0.0f;
#pragma unroll
            for (int t = 0; t < EPH; ++t) {
                float lo = e[t], hi = e[EPH + t];
                asm volatile("" : "+v"(lo), "+v"(hi));     // keep both in VGPRs: a select of two array slots would go to scratch
                E[t] = hh ? hi : lo;
            }
        }
}

// Positions, trilinear gather and Fourier embedding for the lane's sample, in two phases so that the gather's 8 x CH/8
// 16-byte loads are in flight while the caller does something else (the f16 build puts its layer-0 barrier there):
//   issue():  position, ATen's unnormalise / floor / corner weights (zero padding = zero weight), the 8 corner rows
//             requested into registers;
//   finish(): X[0..CH/2) = interpolated grid channels [hh*CH/2, (hh+1)*CH/2), X[CH/2 .. CH/2 + EP/2) = this lane half's
//             share of [p | sin f_k p | cos f_k p | 0 pad].
// Corner offsets are 32-bit (the host entry refuses grids of 4 GiB or more); all conditions are evaluated as masks,
// not short-circuit branches.
template <int CH, int NF>
struct LfgcSampler {
    static constexpr LfgcPlan P = LfgcShape<CH, 1, NF>::P;      // the input side does not depend on the hidden width
    static constexpr int CHH = P.CHH(), EPH = P.EPH();
    float p0, p1, p2;
    float w[8];
    f32x4 v[8][CHH / 4];

    __device__ __forceinline__ void issue(const LfgcFwdArgs& a, long long nc, long long N, const float* s_coord, int hh) {
        // ---- positions ---------------------------------------------------------------------------
        if (a.pos) {
            const float* pp = a.pos + 3 * nc;
            p0 = pp[0]; p1 = pp[1]; p2 = pp[2];
        } else {
            int vx, vy, vz;
            if (N <= 0xffffffffLL) {                          // 32-bit index arithmetic (any slab up to 1625^3)
                const unsigned plane = (unsigned)a.res1 * (unsigned)a.res2;
                const unsigned un = (unsigned)nc;
                const unsigned qx = un / plane, rem = un - qx * plane;
                const unsigned qy = rem / (unsigned)a.res2;
                vx = a.x_begin + (int)qx; vy = (int)qy; vz = (int)(rem - qy * (unsigned)a.res2);
            } else {
                const long long plane = (long long)a.res1 * a.res2;
                vx = a.x_begin + (int)(nc / plane);
                const long long rem = nc % plane;
                vy = (int)(rem / a.res2); vz = (int)(rem % a.res2);
            }
            if (a.coord_table) {
                p0 = s_coord[vx]; p1 = s_coord[a.res0 + vy]; p2 = s_coord[a.res0 + a.res1 + vz];
            } else {
                p0 = lfgc_lattice_coord(vx, a.res0, a.tile, a.scale0);
                p1 = lfgc_lattice_coord(vy, a.res1, a.tile, a.scale1);
                p2 = lfgc_lattice_coord(vz, a.res2, a.tile, a.scale2);
            }
        }
        // ---- trilinear gather: lane (j, hh) interpolates channels [hh*CHH, (hh+1)*CHH) -------------
        // literal copy of lfgc_axis_cell + inside() + clamped() (lfgc_trilinear.h): this statement order pins the kernel's code
        const float ix = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(p0, 1.0f), (float)a.W), 1.0f), 0.5f);
        const float iy = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(p1, 1.0f), (float)a.H), 1.0f), 0.5f);
        const float iz = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(p2, 1.0f), (float)a.D), 1.0f), 0.5f);
        const float fx0 = floorf(ix), fy0 = floorf(iy), fz0 = floorf(iz);
        // clamped to [-2, size] before the conversion: absurd / NaN positions stay defined, and every corner of such a
        // sample is then out of bounds (weight 0) by the index test alone
        const int x0 = (int)fminf(fmaxf(fx0, -2.0f), (float)a.W);
        const int y0 = (int)fminf(fmaxf(fy0, -2.0f), (float)a.H);
        const int z0 = (int)fminf(fmaxf(fz0, -2.0f), (float)a.D);
        float wx[2], wy[2], wz[2];
        wx[1] = __fsub_rn(ix, fx0); wx[0] = __fsub_rn(__fadd_rn(fx0, 1.0f), ix);
        wy[1] = __fsub_rn(iy, fy0); wy[0] = __fsub_rn(__fadd_rn(fy0, 1.0f), iy);
        wz[1] = __fsub_rn(iz, fz0); wz[0] = __fsub_rn(__fadd_rn(fz0, 1.0f), iz);
        unsigned ox[2], oy[2], oz[2];                   // BYTE offsets (32-bit: one SGPR base + one VGPR offset per load)
        const unsigned cell = 4u * (unsigned)a.Cs, row = (unsigned)a.W * cell, plane = (unsigned)a.H * row;
#pragma unroll
        for (int d = 0; d < 2; ++d) {          // out-of-bounds corner = zero weight on that axis; its (clamped) row is still read
            wx[d] = ((unsigned)(x0 + d) < (unsigned)a.W) ? wx[d] : 0.0f;
            wy[d] = ((unsigned)(y0 + d) < (unsigned)a.H) ? wy[d] : 0.0f;
            wz[d] = ((unsigned)(z0 + d) < (unsigned)a.D) ? wz[d] : 0.0f;
            ox[d] = (unsigned)min(max(x0 + d, 0), a.W - 1) * cell + (unsigned)(hh * CHH * 4);
            oy[d] = (unsigned)min(max(y0 + d, 0), a.H - 1) * row;
            oz[d] = (unsigned)min(max(z0 + d, 0), a.D - 1) * plane;
        }
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const int dz = corner >> 2, dy = (corner >> 1) & 1, dx = corner & 1;   // ATen order: tnw, tne, tsw, tse, bnw, ...
            w[corner] = __fmul_rn(__fmul_rn(wx[dx], wy[dy]), wz[dz]);
#if !(LFGC_ABLATE & 1)
            const float* gp = reinterpret_cast<const float*>(reinterpret_cast<const char*>(a.grid) + (oz[dz] + oy[dy] + ox[dx]));
#pragma unroll
            for (int c4 = 0; c4 < CHH / 4; ++c4) v[corner][c4] = *reinterpret_cast<const f32x4*>(gp + 4 * c4);
#else
#pragma unroll
            for (int c4 = 0; c4 < CHH / 4; ++c4) v[corner][c4] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#endif
        }
    }

    __device__ __forceinline__ void finish(int hh, float (&B0)[CHH + EPH]) {
        lfgc_embed_inputs<NF>(p0, p1, p2, hh, B0 + CHH);
        // ---- the 8 corner rows, accumulated in ATen's corner order -----------------------------------
        float feat[CHH];
#pragma unroll
        for (int c = 0; c < CHH; ++c) feat[c] = 0.0f;
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
#pragma unroll
            for (int c4 = 0; c4 < CHH / 4; ++c4) {
                const f32x4 q = v[corner][c4];
                feat[4 * c4 + 0] = __builtin_fmaf(q.x, w[corner], feat[4 * c4 + 0]);
                feat[4 * c4 + 1] = __builtin_fmaf(q.y, w[corner], feat[4 * c4 + 1]);
                feat[4 * c4 + 2] = __builtin_fmaf(q.z, w[corner], feat[4 * c4 + 2]);
                feat[4 * c4 + 3] = __builtin_fmaf(q.w, w[corner], feat[4 * c4 + 3]);
            }
        }
#pragma unroll
        for (int c = 0; c < CHH; ++c) B0[c] = feat[c];
    }
};

// Lattice mode, "z-run" tiles: the 32 samples of a wave are 32 consecutive z voxels of ONE (x, y) row of the volume, so
// they share their x and y cells and weights and together touch only a short COLUMN of the grid: the cells
// zc_lo .. zc_lo + nzc - 1 along z at the four (x, y) corners (nzc = floor(31 D / (res2 - 1)) + 3: 10 cells of the 64-cell
// axis for a 256-voxel row, against 32 samples x 8 corner rows read one by one by LfgcSampler).  The wave
//   stage_a: forms the positions and ATen's weights as LfgcSampler does, then -- 64 lanes = cells x 4-channel quads --
//            loads the four (x, y) corner rows of every cell of the column (4 x dwordx4 per lane and pass instead of 32),
//            contracts them with the x-y weights (ATen's corner order nw, ne, sw, se; the z weight is applied afterwards,
//            once per plane: a different but equally short rounding sequence) and leaves the column in LDS;
//   stage_b: every lane reads the two planes of ITS sample back (2 x CH/8 ds_read_b128) and applies the z weights.
// 16 + 32 FMAs per lane instead of 128, 4-8 vector loads per lane instead of 32, and the loads go out once per cell
// instead of once per sample: the texture-address path, which the 8 waves of a workgroup used to fill for 4 k cycles per
// batch (32 x 8 x 1 KiB through 64 B / clock), is nearly idle.  Lanes whose cell index lies past the column redo one of
// its cells (same value to the same LDS address): no lane predicate, no branch.
constexpr int LFGC_NZC_MAX = 12;                    // longest column (z cells) the host selects this path for
template <int CH, int NF>
struct LfgcColumnSampler {
    static constexpr LfgcPlan P = LfgcShape<CH, 1, NF>::P;
    static constexpr int CHH = P.CHH(), EPH = P.EPH();
    static constexpr int LPC = CH / 4;              // lanes per cell: one 4-channel quad each
    static constexpr int CPP = 64 / LPC;            // cells per pass of the wave
    static constexpr int NZC_MAX = LFGC_NZC_MAX;
    static constexpr int NPASS = (NZC_MAX + CPP - 1) / CPP;
    // LDS row of one column cell: CH floats + 4 of padding -- with 128-byte rows, rows r and r + 2 start on the same bank
    // and the read-back (16 lanes of a ds_read_b128 group spread over 4-5 neighbouring rows) conflicted 2-3 ways
    static constexpr int CS = P.col_row();
    float p0, p1, p2;
    float wz0, wz1;
    int zrel;                                       // (z cell of the sample) - zc_lo, in [0, nzc - 2]
    int q, kcell[NPASS];                            // the lane's channel quad and column cell per pass
    float wxy_[4];
    f32x4 v[NPASS][4];                              // corner quads in flight between stage_a and stage_b

    // vx, vy: the row (wave-uniform); vz: the lane's voxel, already clamped to the row.  s_col: this wave's nzc x CH floats.
    __device__ __forceinline__ void stage_a(const LfgcFwdArgs& a, int vx, int vy, int vz, const float* s_coord,
                                            float* s_col, int lane) {
        p0 = s_coord[vx]; p1 = s_coord[a.res0 + vy]; p2 = s_coord[a.res0 + a.res1 + vz];
        // literal copy of lfgc_axis_cell + inside() + clamped() (lfgc_trilinear.h): this statement order pins the kernel's code
        const float ix = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(p0, 1.0f), (float)a.W), 1.0f), 0.5f);
        const float iy = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(p1, 1.0f), (float)a.H), 1.0f), 0.5f);
        const float iz = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(p2, 1.0f), (float)a.D), 1.0f), 0.5f);
        const float fx0 = floorf(ix), fy0 = floorf(iy), fz0 = floorf(iz);
        const int x0 = (int)fminf(fmaxf(fx0, -2.0f), (float)a.W);
        const int y0 = (int)fminf(fmaxf(fy0, -2.0f), (float)a.H);
        const int z0 = (int)fminf(fmaxf(fz0, -2.0f), (float)a.D);
        float wx[2], wy[2];
        wx[1] = __fsub_rn(ix, fx0); wx[0] = __fsub_rn(__fadd_rn(fx0, 1.0f), ix);
        wy[1] = __fsub_rn(iy, fy0); wy[0] = __fsub_rn(__fadd_rn(fy0, 1.0f), iy);
        wz1 = __fsub_rn(iz, fz0); wz0 = __fsub_rn(__fadd_rn(fz0, 1.0f), iz);
        unsigned ox[2], oy[2];
        const unsigned cell = 4u * (unsigned)a.Cs, row = (unsigned)a.W * cell, plane = (unsigned)a.H * row;
#pragma unroll
        for (int d = 0; d < 2; ++d) {          // out-of-bounds corner = zero weight on that axis; its (clamped) row is still read
            wx[d] = ((unsigned)(x0 + d) < (unsigned)a.W) ? wx[d] : 0.0f;
            wy[d] = ((unsigned)(y0 + d) < (unsigned)a.H) ? wy[d] : 0.0f;
            ox[d] = (unsigned)min(max(x0 + d, 0), a.W - 1) * cell;
            oy[d] = (unsigned)min(max(y0 + d, 0), a.H - 1) * row;
        }
        wz0 = ((unsigned)z0 < (unsigned)a.D) ? wz0 : 0.0f;
        wz1 = ((unsigned)(z0 + 1) < (unsigned)a.D) ? wz1 : 0.0f;
        const int zc_lo = __builtin_amdgcn_readfirstlane(z0);          // lane 0 holds the row's smallest z
        zrel = min(max(z0 - zc_lo, 0), a.nzc - 2);
        const float wxy[4] = {__fmul_rn(wx[0], wy[0]), __fmul_rn(wx[1], wy[0]), __fmul_rn(wx[0], wy[1]), __fmul_rn(wx[1], wy[1])};
        const unsigned oxy[4] = {oy[0] + ox[0], oy[0] + ox[1], oy[1] + ox[0], oy[1] + ox[1]};
        q = lane % LPC;
        const int kl = lane / LPC;
        const float inv_nzc = 1.0f / (float)a.nzc;
#pragma unroll
        for (int c = 0; c < 4; ++c) wxy_[c] = wxy[c];
        // every pass's corner quads are requested here and contracted in stage_b: their latency runs under the embedding
        // arithmetic and the layer-0 barrier instead of being waited out pass by pass
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            int k = ps * CPP + kl;                                     // < NPASS * CPP + 64 / LPC <= 64: exact in fp32
            k -= a.nzc * (int)(((float)k + 0.5f) * inv_nzc);           // k mod nzc
            kcell[ps] = k;
            const int zc = min(max(zc_lo + k, 0), a.D - 1);
            const unsigned off = (unsigned)zc * plane + (unsigned)(q * 16);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                v[ps][c] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(a.grid) + (off + oxy[c]));
        }
    }

    __device__ __forceinline__ void stage_b(float* s_col, int hh, float (&B0)[CHH + EPH]) {
        lfgc_embed_inputs<NF>(p0, p1, p2, hh, B0 + CHH);
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc.x = __builtin_fmaf(v[ps][c].x, wxy_[c], acc.x); acc.y = __builtin_fmaf(v[ps][c].y, wxy_[c], acc.y);
                acc.z = __builtin_fmaf(v[ps][c].z, wxy_[c], acc.z); acc.w = __builtin_fmaf(v[ps][c].w, wxy_[c], acc.w);
            }
            *reinterpret_cast<f32x4*>(s_col + kcell[ps] * CS + 4 * q) = acc;
        }
        const float* c0 = s_col + zrel * CS + hh * CHH;
#pragma unroll
        for (int c4 = 0; c4 < CHH / 4; ++c4) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(c0 + 4 * c4);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(c0 + CS + 4 * c4);
            B0[4 * c4 + 0] = __builtin_fmaf(hi.x, wz1, __fmul_rn(lo.x, wz0));
            B0[4 * c4 + 1] = __builtin_fmaf(hi.y, wz1, __fmul_rn(lo.y, wz0));
            B0[4 * c4 + 2] = __builtin_fmaf(hi.z, wz1, __fmul_rn(lo.z, wz0));
            B0[4 * c4 + 3] = __builtin_fmaf(hi.w, wz1, __fmul_rn(lo.w, wz0));
        }
    }
};

template <int CH, int NF>
__device__ __forceinline__ void lfgc_sample_inputs(const LfgcFwdArgs& a, long long nc, long long N, const float* s_coord,
                                               int hh, float (&B0)[LfgcShape<CH, 1, NF>::P.KS0]) {
    LfgcSampler<CH, NF> sm;
    sm.issue(a, nc, N, s_coord, hh);
    sm.finish(hh, B0);
}

// One hidden layer on a 32-sample tile held in registers.
//   s_blk : LDS block [W (32*MT rows x S floats) | bias 32*MT]
//   Bin   : KS activations of this lane (k order above);  Bout : 16*MT outputs (same order)
//   stash : this layer's slot for the tile: [(m*16 + r)][64 lanes]  (STASH builds only)
template <int KS, int MT, int S, bool STASH>
__device__ __forceinline__ void lfgc_layer_fwd(const float* __restrict__ s_blk, const float (&Bin)[KS],
                                               float (&Bout)[16 * MT], float* __restrict__ stash,
                                               int j, int hh, int lane) {
    static_assert(KS % 4 == 0, "k-steps come in groups of 4 (one ds_read_b128)");
    const float* s_bias = s_blk + 32 * MT * S + 4 * hh;
    const float* s_row = s_blk + j * S + 4 * hh;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(s_bias + 32 * m + 8 * q);
            acc[4 * q + 0] = b4.x; acc[4 * q + 1] = b4.y; acc[4 * q + 2] = b4.z; acc[4 * q + 3] = b4.w;
        }
        const float* arow = s_row + 32 * m * S;
#pragma unroll
        for (int qb = 0; qb < KS / 4; ++qb) {
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(arow + 8 * qb);
#if LFGC_ABLATE & 4
            acc[qb & 15] += a4.x * Bin[4 * qb] + a4.y * Bin[4 * qb + 1] + a4.z * Bin[4 * qb + 2] + a4.w * Bin[4 * qb + 3];
#else
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, Bin[4 * qb + 0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, Bin[4 * qb + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, Bin[4 * qb + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, Bin[4 * qb + 3], acc, 0, 0, 0);
#endif
        }
        if (STASH) {
            // one opaque row pointer per tile + immediate offsets (r * 256 B): otherwise hipcc hoists a 64-bit
            // address per store out of the batch loop and spills ~60 VGPRs
            float* pm = stash + m * (16 * 64) + lane;
            asm volatile("" : "+v"(pm));
#pragma unroll
            for (int r = 0; r < 16; ++r) pm[r * 64] = acc[r];
        }
        float amax = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r += 2) amax = lfgc_absmax3(amax, acc[r], acc[r + 1]);
#if LFGC_ABLATE & 2
#pragma unroll
        for (int r = 0; r < 16; ++r) Bout[16 * m + r] = 0.5f * acc[r];
        amax = 0.0f;
#else
#pragma unroll
        for (int r = 0; r < 16; ++r) Bout[16 * m + r] = lfgc_snake_t<false>(acc[r]);
#endif
        if (__builtin_expect(__any(amax > LFGC_TRIG_FAST_MAX), 0)) {       // wave-uniform; a diverged model only
#pragma unroll
            for (int r = 0; r < 16; ++r) Bout[16 * m + r] = lfgc_snake_t<true>(acc[r]);
        }
    }
}

// Dynamic LDS of lfgc_fwd_kernel in floats, in the order the kernel carves it:
//   s_final [Wf (HP) | bf (4)] | s_w: every layer block (resident) or a ring of 2 slots of the larger block (streamed)
//   | s_coord: the per-axis coordinate tables, `table_floats` = res0 + res1 + res2 (lattice mode, where they fit; else 0).
// The host's launch selection sizes the allocation with these functions and the kernel static_asserts its pointers
// against them.
constexpr int lfgc_fwd_lds_head(const LfgcPlan& p) { return p.HP + 4; }
constexpr int lfgc_fwd_lds_ring_slot(const LfgcPlan& p) { return p.blk0 > p.blk1 ? p.blk0 : p.blk1; }
constexpr long long lfgc_fwd_lds_floats(const LfgcPlan& p, bool resident, long long table_floats) {
    return lfgc_fwd_lds_head(p) + (resident ? p.off_final : 2 * lfgc_fwd_lds_ring_slot(p)) + table_floats;
}

// STREAM = false: WAVES = 4, two workgroups per CU, layer blocks staged once ("resident" nets that fit 80 KB of LDS).
// STREAM = true : one workgroup per CU, the layer blocks stream through a 2-deep LDS ring by LDS-DMA: the block of
//            layer t+1 is in flight while layer t computes, one barrier per layer, no exposed staging.  WAVES = 8
//            (256 samples per batch) when there are enough batches to give every CU one, else WAVES = 4 so that a
//            32 768-sample call (one reference tile / train step) still spreads over all 256 CUs.
template <int CH, int MT, int NF, int WAVES, bool STREAM, bool STASH>
__global__ __launch_bounds__(WAVES * 64, 2) void lfgc_fwd_kernel(const LfgcFwdArgs a) {
    using SHAPE = LfgcShape<CH, MT, NF>;
    constexpr LfgcPlan P = SHAPE::P;
    constexpr int HP = P.HP, KS0 = P.KS0, KS1 = P.KS1, S0 = P.S0, S1 = P.S1, blk0 = P.blk0, blk1 = P.blk1;
    constexpr int BLKMAX = lfgc_fwd_lds_ring_slot(P);
    constexpr int NT = WAVES * 64;

    // range fallback of the f16 builds: nothing to redo (uniform).  Device-scope load: the word is written by the kernel
    // enqueued just before this one (and cleared by lfgc_clear_word_kernel before that), possibly through another XCD's L2
    if (a.redo_if && __hip_atomic_load(a.redo_if, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_final = smem;               // Wf (HP) | bf (4)
    constexpr int HEAD = lfgc_fwd_lds_head(P);
    float* s_w = smem + HEAD;            // resident: every layer block; streamed: ring of 2 x BLKMAX
    // lattice mode: coordinate of every voxel index per axis, built once per workgroup (the per-sample form
    // costs two fp64 divisions per axis); placed behind the weight region
    float* s_coord = s_w + (STREAM ? 2 * BLKMAX : (blk0 + (a.L - 1) * blk1));
    static_assert(HEAD == HP + 4, "s_final is [Wf (HP) | bf (4)]");
    static_assert(lfgc_fwd_lds_floats(P, false, 0) == HEAD + 2 * BLKMAX, "streamed: s_coord follows the ring");
    constexpr auto resident_floats_of = [](int L) { return HEAD + (blk0 + (L - 1) * blk1); };
    static_assert(resident_floats_of(1) == lfgc_fwd_lds_floats(SHAPE::P, true, 0) &&
                  resident_floats_of(LFGC_MAX_LAYERS) == lfgc_fwd_lds_floats(SHAPE::PL, true, 0), "resident: s_coord follows the blocks");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int j = lane & 31;
    const int hh = lane >> 5;
    const int L = a.L;
    const int off_final = blk0 + (L - 1) * blk1;
    constexpr auto off_final_of = [](int L) { return blk0 + (L - 1) * blk1; };
    LFGC_ASSERT_PLAN_OFFSET(SHAPE, off_final_of, off_final);
    constexpr auto stash_tile_of = [](int L) { return 64 * (KS0 + L * 16 * MT); };
    LFGC_ASSERT_PLAN_OFFSET(SHAPE, stash_tile_of, stash_tile_floats);

    {   // final layer (+ every layer block when resident): staged once per workgroup
        const f32x4* src = reinterpret_cast<const f32x4*>(a.packed + off_final);
        for (int i = tid; i < (HP + 4) / 4; i += NT) reinterpret_cast<f32x4*>(s_final)[i] = src[i];
        if (!STREAM) {
            const f32x4* srcw = reinterpret_cast<const f32x4*>(a.packed);
            for (int i = tid; i < off_final / 4; i += NT) reinterpret_cast<f32x4*>(s_w)[i] = srcw[i];
        } else {
            lfgc_dma_to_lds(a.packed, s_w, blk0, wave, lane, WAVES);      // layer 0 of the first batch -> slot 0
        }
    }
    if (!a.pos && a.coord_table) lfgc_fill_coord_table(a, s_coord, tid, NT);
    __syncthreads();
    unsigned step = 0;                   // streamed: layers executed so far (ring slot = step & 1)

    const long long N = a.n;
    for (long long batch = blockIdx.x; batch < a.nbatches; batch += gridDim.x) {
        const long long tile_idx = batch * WAVES + wave;
        const long long n = tile_idx * LFGC_TILE_SAMPLES + j;
        const bool valid = n < N;
        const long long nc = valid ? n : (N - 1);

        float B0[KS0];
        lfgc_sample_inputs<CH, NF>(a, nc, N, s_coord, hh, B0);

        float* stash_tile = nullptr;
        if (STASH) {
            stash_tile = a.stash + tile_idx * (long long)(64 * (KS0 + L * 16 * MT));
            {
                float* px = stash_tile + lane;
                asm volatile("" : "+v"(px));
#pragma unroll
                for (int s = 0; s < KS0; ++s) px[s * 64] = B0[s];
            }
            stash_tile += 64 * KS0;
        }

        // ---- layers ------------------------------------------------------------------------------------
        // streamed: this layer's block was put in flight one step ago: wait for my pieces, then for everyone's;
        // the same barrier says every wave is done with the other ring slot -> prefetch the next block into it
        auto acquire = [&](int l) -> const float* {
            if (!STREAM) return s_w + (l == 0 ? 0 : blk0 + (l - 1) * blk1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            const float* blk = s_w + (step & 1) * BLKMAX;
            const int ln = (l + 1 == L) ? 0 : l + 1;
            if (ln != 0 || batch + gridDim.x < a.nbatches) {
                const float* src = a.packed + (ln == 0 ? 0 : blk0 + (long long)(ln - 1) * blk1);
                lfgc_dma_to_lds(src, s_w + ((step + 1) & 1) * BLKMAX, ln == 0 ? blk0 : blk1, wave, lane, WAVES);
            }
            ++step;
            return blk;
        };
        float Bn[16 * MT];
        {
            const float* blk = acquire(0);
            lfgc_layer_fwd<KS0, MT, S0, STASH>(blk, B0, Bn, stash_tile, j, hh, lane);
        }
        // hidden layers two at a time, ping-ponging between two register arrays (no per-layer copy)
        {
            float Bm[16 * MT];
            int l = 1;
            for (; l + 1 < L; l += 2) {
                const float* blk = acquire(l);
                lfgc_layer_fwd<KS1, MT, S1, STASH>(blk, Bn, Bm, STASH ? stash_tile + (long long)l * P.stash_layer_floats() : nullptr,
                                                   j, hh, lane);
                blk = acquire(l + 1);
                lfgc_layer_fwd<KS1, MT, S1, STASH>(blk, Bm, Bn, STASH ? stash_tile + (long long)(l + 1) * P.stash_layer_floats() : nullptr,
                                                   j, hh, lane);
            }
            if (l < L) {
                const float* blk = acquire(l);
                lfgc_layer_fwd<KS1, MT, S1, STASH>(blk, Bn, Bm, STASH ? stash_tile + (long long)l * P.stash_layer_floats() : nullptr,
                                                   j, hh, lane);
#pragma unroll
                for (int s = 0; s < KS1; ++s) Bn[s] = Bm[s];
            }
        }

        // ---- final Linear (H -> 1): per-lane partial dot + exchange between the two lane halves ------
        float y = 0.0f;
#pragma unroll
        for (int qb = 0; qb < KS1 / 4; ++qb) {
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(s_final + 8 * qb + 4 * hh);
            y = __builtin_fmaf(w4.x, Bn[4 * qb + 0], y);
            y = __builtin_fmaf(w4.y, Bn[4 * qb + 1], y);
            y = __builtin_fmaf(w4.z, Bn[4 * qb + 2], y);
            y = __builtin_fmaf(w4.w, Bn[4 * qb + 3], y);
        }
        y += __shfl_xor(y, 32);
        y += s_final[HP];
        if (a.clamp) y = fminf(fmaxf(y, -1.0f), 1.0f);
        if (valid && hh == 0) a.out[n] = y;
    }
}

// Host-side launcher for one (CH, MT) pair: picks the resident (4-wave) or streamed (8-wave) build and the
// stash / no-stash build.
template <int CH, int MT, int NF, int WAVES, bool STREAM, bool STASH>
static int lfgc_launch_fwd_one(const LfgcFwdArgs& a, int lds_bytes, int grid, hipStream_t stream) {
    return lfgc_launch<lfgc_fwd_kernel<CH, MT, NF, WAVES, STREAM, STASH>>(dim3(grid), dim3(WAVES * 64), lds_bytes, stream, a);
}

template <int CH, int MT, int NF>
static int lfgc_launch_fwd(const LfgcFwdArgs& a, int lds_bytes, int grid, hipStream_t stream) {
    if (a.resident) {
        return a.stash ? lfgc_launch_fwd_one<CH, MT, NF, 4, false, true>(a, lds_bytes, grid, stream)
                       : lfgc_launch_fwd_one<CH, MT, NF, 4, false, false>(a, lds_bytes, grid, stream);
    }
    if (a.waves == 8) {
        return a.stash ? lfgc_launch_fwd_one<CH, MT, NF, 8, true, true>(a, lds_bytes, grid, stream)
                       : lfgc_launch_fwd_one<CH, MT, NF, 8, true, false>(a, lds_bytes, grid, stream);
    }
    return a.stash ? lfgc_launch_fwd_one<CH, MT, NF, 4, true, true>(a, lds_bytes, grid, stream)
                   : lfgc_launch_fwd_one<CH, MT, NF, 4, true, false>(a, lds_bytes, grid, stream);
}
