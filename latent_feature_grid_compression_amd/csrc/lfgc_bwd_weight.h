// lfgc_bwd_weight.h -- the backward's weight-gradient kernel (kernel 2 of lfgc_backward.h) and the launch of the training
// backward: data kernel, deferred scatter if asked for, weight kernel.
#pragma once
#include "lfgc_bwd_data.h"

// The 16 samples a lane contributes to a tile's contraction: [8 kh, 8 kh + 8) and [16 + 8 kh, 16 + 8 kh + 8) of stash row
// `base` (= row start + lane-half offset): exactly the k values lane half kh feeds to the two 16-deep k-steps of
// v_mfma_f32_32x32x16_f16 (and, pairwise with the other half, to 16 v_mfma_f32_32x32x2_f32).
__device__ __forceinline__ void lfgc_load16(const float* __restrict__ base, int kh, float (&v)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(base + 8 * kh + 16 * (q >> 1) + 4 * (q & 1));
        v[4 * q + 0] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
}

// h[i] = snake(a[i]) for a wave's tile of stashed pre-activations: the whole tile with the fast reduction, redone with the
// wide one under one wave-uniform branch if any lane was out of range (`a` and `h` are different arrays).
template <int N>
__device__ __forceinline__ void lfgc_snake_tile(const float (&a)[N], float (&h)[N]) {
    bool bad = false;
#pragma unroll
    for (int s = 0; s < N; ++s) bad |= lfgc_trig_out_of_range(a[s]);
#pragma unroll
    for (int s = 0; s < N; ++s) h[s] = lfgc_snake_t<false>(a[s]);
    if (__builtin_expect(__any(bad), 0)) {
#pragma unroll
        for (int s = 0; s < N; ++s) h[s] = lfgc_snake_t<true>(a[s]);
    }
}

// One layer's dW (+ db) over this workgroup's sample tiles.  NT = column tiles of this layer, KSIN = stash
// registers of the input (KS0 for layer 0 where the input is the saved x0, else 16*MT pre-activations).
// The workgroup has 8 waves: waves 0-3 and 4-7 run the same tile/column assignment on alternate sample tiles (two
// waves per SIMD, so one wave's loads hide under the other's MFMAs); the second half hands its accumulators over
// through LDS (`s_comb`, [4 waves][TPW*17][64]) and the first half writes the slab.
// Contraction over the 32 samples of a tile: with a.dscale (the f16 builds) as f16 hi/lo split operands, three
// v_mfma_f32_32x32x16_f16 per 16 samples with fp32 accumulation -- dA scaled by the power of two the data kernel chose for
// the tile, the tile's product scaled back exactly before it joins the running sum --, 192 instead of 1024 matrix-pipe
// cycles per 32x32 output tile; a tile whose inputs leave the f16 range (|H| >= 65504: a diverged model), and the exact
// build, take sixteen v_mfma_f32_32x32x2_f32 (bitwise an fp32 fmaf chain).
template <int MT, int NT, bool LAYER0, int KS0>
__device__ __forceinline__ void lfgc_wgrad_layer(const LfgcWgradArgs& a, int l, float* __restrict__ slab_l, int ncol,
                                                 int k0p, long long per_tile, long long dper_tile,
                                                 int lane, int wave8, float* s_comb, int grp, int ngrp) {
    const int half = wave8 >> 2, wave = wave8 & 3;
    constexpr int WPN = 4 / NT;                       // waves sharing one column tile
    constexpr int TPW = (MT + WPN - 1) / WPN;         // row tiles per wave
    const int n_t = wave % NT, msub = wave / NT;
    const int i = lane & 31, kk = lane >> 5;
    f32x16 acc[TPW];
    float dbp[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        dbp[t] = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    }
    // B operand row for this lane: column col = 32 n_t + i of the layer input
    const int col = 32 * n_t + i;
    long long boff;
    bool bvalid = true;
    if (LAYER0) {
        const int s = 4 * (col >> 3) + (col & 3), hb = (col >> 2) & 1;
        bvalid = col < k0p;
        boff = (long long)(bvalid ? s : 0) * 64 + hb * 32;
    } else {
        const int r = (i & 3) + 4 * (i >> 3), hb = (i >> 2) & 1;
        boff = 64LL * KS0 + (long long)(l - 1) * (64 * 16 * MT) + (long long)(n_t * 16 + r) * 64 + hb * 32;
    }
    // A operand rows: row = 32 m + i of dA_l
    const int ra = (i & 3) + 4 * (i >> 3), ha = (i >> 2) & 1;
    const long long aoff_base = (long long)l * (64 * 16 * MT) + (long long)ra * 64 + ha * 32;

    for (long long t = grp + (long long)half * ngrp; t < a.ntiles; t += 2LL * ngrp) {
        float Bv[16];
        lfgc_load16(a.stash + t * per_tile + boff, kk, Bv);
        if (LAYER0) {
            if (!bvalid) {
#pragma unroll
                for (int s = 0; s < 16; ++s) Bv[s] = 0.0f;
            }
        } else {
            float Hv[16];
            lfgc_snake_tile(Bv, Hv);
#pragma unroll
            for (int s = 0; s < 16; ++s) Bv[s] = Hv[s];
        }
        bool split = a.dscale != nullptr;
        float sc = 1.0f, isc = 1.0f;
        h16x8 Bhi[2], Blo[2];
        if (split) {
            float bmax = 0.0f;
#pragma unroll
            for (int s = 0; s < 16; s += 2) bmax = lfgc_absmax3(bmax, Bv[s], Bv[s + 1]);
            split = !__any(!(bmax < 65504.0f));                    // wave-uniform; NaN / inf / huge inputs -> exact path
            sc = a.dscale[t * a.L + l];
            isc = __int_as_float(0x7F000000 - __float_as_int(sc));  // 1 / 2^k, exact
            lfgc_split8(Bv, Bhi[0], Blo[0]);
            lfgc_split8(Bv + 8, Bhi[1], Blo[1]);
        }
#pragma unroll
        for (int tw = 0; tw < TPW; ++tw) {
            const int m = msub + tw * WPN;
            if (m < MT) {
                float Av[16];
                lfgc_load16(a.dstash + t * dper_tile + aoff_base + (long long)m * (16 * 64), kk, Av);
#pragma unroll
                for (int s = 0; s < 16; ++s) dbp[tw] += Av[s];
                if (split) {
                    float As[16];
#pragma unroll
                    for (int s = 0; s < 16; ++s) As[s] = Av[s] * sc;
                    h16x8 Ahi[2], Alo[2];
                    lfgc_split8(As, Ahi[0], Alo[0]);
                    lfgc_split8(As + 8, Ahi[1], Alo[1]);
                    f32x16 tmp;
#pragma unroll
                    for (int r = 0; r < 16; ++r) tmp[r] = 0.0f;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        tmp = __builtin_amdgcn_mfma_f32_32x32x16_f16(Alo[ks], Bhi[ks], tmp, 0, 0, 0);
                        tmp = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ahi[ks], Blo[ks], tmp, 0, 0, 0);
                        tmp = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ahi[ks], Bhi[ks], tmp, 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[tw][r] = __builtin_fmaf(tmp[r], isc, acc[tw][r]);
                } else {
#pragma unroll
                    for (int s = 0; s < 16; ++s)
                        acc[tw] = __builtin_amdgcn_mfma_f32_32x32x2f32(Av[s], Bv[s], acc[tw], 0, 0, 0);
                }
            }
        }
    }
    // second half -> LDS -> first half
    float* mine = s_comb + (long long)wave * (TPW * 17 * 64) + lane;
    if (half == 1) {
#pragma unroll
        for (int tw = 0; tw < TPW; ++tw) {
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[(tw * 17 + r) * 64] = acc[tw][r];
            mine[(tw * 17 + 16) * 64] = dbp[tw];
        }
    }
    __syncthreads();
    if (half == 0) {
#pragma unroll
        for (int tw = 0; tw < TPW; ++tw) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tw][r] += mine[(tw * 17 + r) * 64];
            dbp[tw] += mine[(tw * 17 + 16) * 64];
        }
    }
    __syncthreads();
    if (half == 1) return;
    // write this workgroup's partial: dW[32m + row][32 n_t + colj], rows from the accumulator layout
    const int cj = lane & 31, hc = lane >> 5;
#pragma unroll
    for (int tw = 0; tw < TPW; ++tw) {
        const int m = msub + tw * WPN;
        if (m < MT) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * hc;
                slab_l[(long long)row * ncol + 32 * n_t + cj] = acc[tw][r];
            }
            const float tot = dbp[tw] + __shfl_xor(dbp[tw], 32);
            if (n_t == 0 && kk == 0) slab_l[(long long)(32 * MT) * ncol + 32 * m + i] = tot;
        }
    }
}

template <int CH, int MT, int NF>
__global__ __launch_bounds__(512, 2) void lfgc_bwd_weight_kernel(const LfgcWgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float s_comb[];
    using SHAPE = LfgcShape<CH, MT, NF>;
    constexpr LfgcPlan P = SHAPE::P;
    constexpr int K0P = P.K0P, K0R = P.K0R, KS0 = P.KS0, HP = P.HP;
    constexpr int NT0 = K0R / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = a.L;
    const long long per_tile = 64LL * (KS0 + L * 16 * MT);
    const long long dper_tile = 64LL * (L * 16 * MT);
    const int R = a.roles;
    const int role = (int)blockIdx.x % R, grp = (int)blockIdx.x / R, ngrp = (int)gridDim.x / R;    // workgroup-uniform
    float* slab = a.slabs + (long long)grp * a.slab_floats;
    // the slab offsets below, written out in l, are lfgc_slab_layer_off's
    constexpr int slab_blk0 = P.slab_blk0(), slab_blk1 = P.slab_blk1();
    constexpr auto slab_off_of = [](int l) { return slab_blk0 + (l - 1) * slab_blk1; };
    static_assert(slab_off_of(1) == lfgc_slab_layer_off(SHAPE::PL, 1) &&
                  slab_off_of(LFGC_MAX_LAYERS) == lfgc_slab_layer_off(SHAPE::PL, LFGC_MAX_LAYERS), "slab layout");
    constexpr auto stash_tile_of = [](int L) { return 64 * (KS0 + L * 16 * MT); };
    LFGC_ASSERT_PLAN_OFFSET(SHAPE, stash_tile_of, stash_tile_floats);

    if (R == 1 || role == 0) lfgc_wgrad_layer<MT, NT0, true, KS0>(a, 0, slab, K0R, K0P, per_tile, dper_tile, lane, wave, s_comb, grp, ngrp);
    for (int l = 1; l < L; ++l) {
        if (R != 1 && role != l) continue;
        float* slab_l = slab + slab_blk0 + (long long)(l - 1) * slab_blk1;
        lfgc_wgrad_layer<MT, MT, false, KS0>(a, l, slab_l, HP, K0P, per_tile, dper_tile, lane, wave, s_comb, grp, ngrp);
    }

    // final Linear: dWf[k] = sum_n dy_n H_L[n,k], dbf = sum_n dy_n.  Wave w owns column tile w.
    if (R == 1 || role == L - 1) {
        float* slab_f = slab + slab_blk0 + (long long)(L - 1) * slab_blk1;
        const int i = lane & 31, kk = lane >> 5;
        const int half = wave >> 2, w4 = wave & 3;
        float wsum = 0.0f, bsum = 0.0f;
        if (w4 < MT) {
            const int r = (i & 3) + 4 * (i >> 3), hb = (i >> 2) & 1;
            const long long boff = 64LL * KS0 + (long long)(L - 1) * P.stash_layer_floats() + (long long)(w4 * 16 + r) * 64 + hb * 32;
            for (long long t = grp + (long long)half * ngrp; t < a.ntiles; t += 2LL * ngrp) {
                float Bv[16], Hv[16];
                lfgc_load16(a.stash + t * per_tile + boff, kk, Bv);
                lfgc_snake_tile(Bv, Hv);
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const long long smp = t * 32 + 8 * kk + 16 * (s >> 3) + (s & 7);       // lfgc_load16's sample order
                    const float dyv = smp < a.n ? a.d_out[smp] : 0.0f;
                    wsum = __builtin_fmaf(dyv, Hv[s], wsum);
                    bsum += dyv;
                }
            }
            wsum += __shfl_xor(wsum, 32);
            bsum += __shfl_xor(bsum, 32);
        }
        if (half == 1) { s_comb[w4 * 128 + lane] = wsum; s_comb[w4 * 128 + 64 + lane] = bsum; }
        __syncthreads();
        if (half == 0 && w4 < MT) {
            wsum += s_comb[w4 * 128 + lane];
            bsum += s_comb[w4 * 128 + 64 + lane];
            if (kk == 0) slab_f[32 * w4 + i] = wsum;
            if (w4 == 0 && lane == 0) slab_f[HP] = bsum;
        }
    }
}

template <int CH, int MT, int NF>
static int lfgc_launch_bwd(const LfgcBwdArgs& a, const LfgcWgradArgs& w, int waves, int h16, int lds_bytes, int grid_data,
                           int grid_w, hipStream_t stream, const LfgcDetScatter* det) {
    int rc = lfgc_launch_bwd_data_any<CH, MT, NF, false>(a, waves, h16, lds_bytes, grid_data, stream);
    if (rc != LFGC_OK) return rc;
    if (a.dfeat) {                                        // deferred scatter of the feature gradients
        const long long blocks = (a.n + 31) / 32;         // 4 waves x 8 samples
        if (det) {                                        // fixed point, integer atomics (the caller zeroes and finishes)
            rc = lfgc_launch_det_max(a.dfeat, a.n * CH, det->maxw, stream);
            if (rc != LFGC_OK) return rc;
            hipLaunchKernelGGL(lfgc_bwd_scatter_det_kernel<CH>, dim3((unsigned)blocks), dim3(256), 0, stream, a.pos, a.dfeat,
                               det->acc, det->maxw, a.n, a.D, a.H, a.W, a.Cs);
        } else {
            hipLaunchKernelGGL(lfgc_bwd_scatter_kernel<CH>, dim3((unsigned)blocks), dim3(256), 0, stream, a.pos, a.dfeat, a.d_grid,
                               a.n, a.D, a.H, a.W, a.Cs);
        }
        LFGC_HIP_CHECK_LAUNCH();
    }
    constexpr int NT0_ = LfgcShape<CH, MT, NF>::P.K0R / 32;
    constexpr int TPW0 = (MT + 4 / NT0_ - 1) / (4 / NT0_), TPW1 = (MT + 4 / MT - 1) / (4 / MT);
    constexpr int TPWM = TPW0 > TPW1 ? TPW0 : TPW1;
    const int comb_bytes = 4 * TPWM * 17 * 64 * 4;
    return lfgc_launch<lfgc_bwd_weight_kernel<CH, MT, NF>>(dim3(grid_w), dim3(512), comb_bytes, stream, w);
}
