// lfgc_bwd_data.h -- the backward's data kernel (kernel 1 of lfgc_backward.h: the chain run backwards, d_grid, d_pos), the
// two kernels of the deferred feature-gradient scatter, and the data kernel's launch.  All the input-gradient build
// (lfgc_igrad_ch*.hip) includes.
#pragma once
#include "lfgc_backward.h"
#include "lfgc_f16split.h"       // h16x8, lfgc_split8, lfgc_cvt8
#include "lfgc_forward.h"        // lfgc_fourier_trig
#include "lfgc_trilinear.h"

#ifdef LFGC_STAMPS
#define LFGC_BSTAMP(k) do { const unsigned long long now__ = __builtin_amdgcn_s_memtime(); bst[k] += now__ - bst_last; bst_last = now__; } while (0)
#else
#define LFGC_BSTAMP(k) do { } while (0)
#endif

// acc += W_tile . B for one 32-row M tile; `arow` = LDS address of (row 32m + lane&31, column 4*(lane>>5)).
template <int KS>
__device__ __forceinline__ f32x16 lfgc_mfma_tile(const float* __restrict__ arow, const float (&Bin)[KS], f32x16 acc) {
    static_assert(KS % 4 == 0, "k-steps come in groups of 4 (one ds_read_b128)");
#pragma unroll
    for (int qb = 0; qb < KS / 4; ++qb) {
        const f32x4 a4 = *reinterpret_cast<const f32x4*>(arow + 8 * qb);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, Bin[4 * qb + 0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, Bin[4 * qb + 1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, Bin[4 * qb + 2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, Bin[4 * qb + 3], acc, 0, 0, 0);
    }
    return acc;
}

// dA[i] = dH[i] * snake'(a[i]) for the 16*MT pre-activations of one layer (a read from the stash slot): the whole tile
// with the fast reduction, redone with the wide one under one wave-uniform branch if any lane was out of range
// (lfgc_snake_tile, lfgc_bwd_weight.h, is the same rule for the activation's value).
template <int MT>
__device__ __forceinline__ void lfgc_snake_bwd(const float* __restrict__ slot, const float (&dH)[16 * MT],
                                               float (&dA)[16 * MT], int lane) {
    float av[16 * MT];
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 16 * MT; ++i) {
        av[i] = slot[i * 64 + lane];
        bad |= lfgc_trig_out_of_range(av[i]);
    }
#pragma unroll
    for (int i = 0; i < 16 * MT; ++i) dA[i] = dH[i] * lfgc_snake_grad_t<false>(av[i]);
    if (__builtin_expect(__any(bad), 0)) {
#pragma unroll
        for (int i = 0; i < 16 * MT; ++i) dA[i] = dH[i] * lfgc_snake_grad_t<true>(av[i]);
    }
}

// acc += Wt_tile . dA for one 32-row tile with f16-split operands (three MFMAs per 16-wide k-step); `arow` = LDS
// address of (row 32m + lane&31, lane half's 32 bytes of k-step 0).
// `dma`: the next image's weight stream (lfgc_dma_piece, lfgc_common.h); pieces [pi0, pi0 + KS16) capped at NPW go out one
// per k-step, in the shadow of its MFMAs, instead of all at once after the layer's barrier (NPW = 0: not streamed here).
template <int KS16, bool SPLIT, int NPW = 0, int WAVES = 4>
__device__ __forceinline__ f32x16 lfgc_mfma_tile16(const float* __restrict__ arow, const h16x8 (&Fhi)[KS16],
                                                   const h16x8 (&Flo)[KS16], f32x16 acc,
                                                   const LfgcDmaPlan* dma = nullptr, int pi0 = 0) {
#pragma unroll
    for (int ks = 0; ks < KS16; ++ks) {
        if constexpr (NPW > 0) { if (pi0 + ks < NPW) lfgc_dma_piece<WAVES>(*dma, pi0 + ks); }
        const h16x8 whi = *reinterpret_cast<const h16x8*>(arow + 16 * ks);
        if (SPLIT) {
            const h16x8 wlo = *reinterpret_cast<const h16x8*>(arow + 16 * ks + 4);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlo, Fhi[ks], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi, Flo[ks], acc, 0, 0, 0);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi, Fhi[ks], acc, 0, 0, 0);   // SPLIT = false: the single product
    }
    return acc;
}

// Gradients span many orders of magnitude and are small: before the f16 hi/lo split each wave scales its 32-sample
// tile of dA by a power of two that brings the tile maximum to [2^13, 2^14) (so that the lo halves, 2^-11 of the hi,
// do not fall off the bottom of the f16 range); the product is scaled back exactly.  Returns the scale, writes 1/scale.
template <int NV>
__device__ __forceinline__ float lfgc_tile_pow2_scale(const float (&v)[NV], float& inv) {
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < NV; i += 2) amax = lfgc_absmax3(amax, v[i], v[i + 1]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
    const int e = (__float_as_int(amax) >> 23) & 255;            // amax = 1.x * 2^(e - 127); e == 0: zero tile
    int k = (e == 0 || e == 255) ? 0 : (13 + 127 - e);
    k = k > 100 ? 100 : (k < -100 ? -100 : k);
    inv = __int_as_float((127 - k) << 23);
    return __int_as_float((127 + k) << 23);
}

template <int NF16, bool SPLIT>
__device__ __forceinline__ void lfgc_split_scaled(const float* __restrict__ v, float sc, h16x8 (&Fhi)[NF16], h16x8 (&Flo)[NF16]) {
#pragma unroll
    for (int f = 0; f < NF16; ++f) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = v[8 * f + u] * sc;
        if (SPLIT) lfgc_split8(t, Fhi[f], Flo[f]);
        else lfgc_cvt8(t, Fhi[f]);
    }
}

// Sampler coordinate gradient of one corner (ATen grid_sampler_3d_backward): the corner's grid row `gp` dotted with this
// lane half's feature gradients, times the other two axes' weights, signed by the corner's side (d = 0: -, 1: +).
template <int CHH>
__device__ __forceinline__ void lfgc_corner_coord_grad(const float* __restrict__ gp, const float* dX, int dx, int dy, int dz,
                                                       float wxc, float wyc, float wzc, float& gix, float& giy, float& giz) {
    float dot = 0.0f;
#pragma unroll
    for (int c4 = 0; c4 < CHH / 4; ++c4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(gp + 4 * c4);
        dot = __builtin_fmaf(v.x, dX[4 * c4 + 0], dot); dot = __builtin_fmaf(v.y, dX[4 * c4 + 1], dot);
        dot = __builtin_fmaf(v.z, dX[4 * c4 + 2], dot); dot = __builtin_fmaf(v.w, dX[4 * c4 + 3], dot);
    }
    gix += (dx ? dot : -dot) * (wyc * wzc);
    giy += (dy ? dot : -dot) * (wxc * wzc);
    giz += (dz ? dot : -dot) * (wxc * wyc);
}

// The blob offsets and tile strides lfgc_bwd_data_kernel spells out at run time, repeated for a given L and compared with
// the plan's (off_img: the exact chain reads the images at off_t, the f16 chains those at off_ht).
template <int CH, int MT, int NF>
constexpr bool lfgc_bwd_offsets_are_the_plans(int L) {
    constexpr LfgcPlan P = LfgcShape<CH, MT, NF>::P;
    constexpr int HP = P.HP, KS0 = P.KS0, blk0 = P.blk0, blk1 = P.blk1, tblk0 = P.tblk0, tblk1 = P.tblk1, blkh0 = P.blkh0, blkh1 = P.blkh1;
    const LfgcPlan q = lfgc_make_plan(CH, HP, L, NF);
    const int off_final = blk0 + (L - 1) * blk1;
    const int off_t = off_final + HP + 4;
    const int off_h = off_t + tblk0 + (L - 1) * tblk1;
    const int off_img16 = off_h + 32 + LFGC_MAX_LAYERS * HP + HP + blkh0 + (L - 1) * blkh1;
    return off_final == q.off_final && off_t == q.off_t && off_h == q.off_h && off_img16 == q.off_ht &&
           64LL * (KS0 + L * 16 * MT) == q.stash_tile_floats && 64LL * (L * 16 * MT) == (long long)L * q.stash_layer_floats();
}

// One workgroup per CU (WAVES = 8 when every CU gets a 256-sample batch, else 4); the transposed weight images
// stream through a 2-deep LDS ring by LDS-DMA exactly like the forward's (image of step t+1 in flight while step
// t computes, one barrier per step); the scatter staging aliases the ring slot that has just been consumed.
// PREC (the C-ABI precision code) 0: exact f32 MFMA chain.  1: the chain's GEMMs run f16-split like the default forward
// build (dA carried as f16 hi+lo fragments, transposed weight images pre-split and scaled; fp32 accumulate, scaled
// back).  2: reduced precision, the hi halves only (one f16 product).
// INPUT_ONLY: the build behind lfgc_input_gradient_f32, d out / d pos and nothing else.  The same chain with the same carve
// and launch geometry, minus everything the parameter gradients need: no dstash and dscale stores, no scatter of the feature
// gradients (no staging, none of its two barriers, no atomics, no dfeat); all of dX0 is always computed, a.d_out may be
// nullptr (dy = 1) and a.d_pos is mandatory.  Every difference is an `if constexpr`, so the training instantiations are the
// kernels they were (DESIGN.md section 3.3 has the resource table).
template <int CH, int MT, int NF, int WAVES, int PREC, bool INPUT_ONLY = false>
__global__ __launch_bounds__(WAVES * 64, 2) void lfgc_bwd_data_kernel(const LfgcBwdArgs a) {
    constexpr bool H16 = PREC != 0;
    constexpr bool SPLIT = PREC == 1;
    using SHAPE = LfgcShape<CH, MT, NF>;
    constexpr LfgcPlan P = SHAPE::P;
    constexpr int E = P.E, K0R = P.K0R, KS0 = P.KS0, HP = P.HP, KS1 = P.KS1, ST = P.ST;
    constexpr int blk0 = P.blk0, blk1 = P.blk1, tblk0 = P.tblk0, tblk1 = P.tblk1;
    constexpr int CHH = P.CHH(), EPH = P.EPH();
    constexpr int TXF = (CHH + 15) / 16;         // M tiles of dX0 that hold grid-feature gradients
    constexpr int TXA = K0R / 32;                // ... all of dX0 (features + scalar inputs)
    constexpr int SCS = P.scatter_row();         // scatter staging row stride (floats)
    constexpr int SC_WAVE = P.scatter_wave();    // per wave: dfeat rows + 8 weights + 8 offsets per sample
    constexpr int SPI = 64 / CH;                 // samples covered by one atomic wave-instruction
    constexpr int TBMAX = tblk0 > tblk1 ? tblk0 : tblk1;
    constexpr int SLOT = lfgc_bwd_lds_slot(P, WAVES);   // ring slot (floats): an image or the scatter staging of every wave
    constexpr int NT = WAVES * 64;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_final = smem;               // Wf (HP) | bf (4)
    float* s_inv = smem + HP + 4;        // 1 / scale per layer (f16-split build), 8 floats
    float* s_ring = s_inv + 8;           // 2 x SLOT: transposed weight images / scatter staging
    static_assert(lfgc_bwd_lds_floats(P, WAVES) == (HP + 4) + 8 + 2 * SLOT && SLOT >= TBMAX && SLOT >= WAVES * SC_WAVE,
                  "this carve is not the one the host sizes");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, hh = lane >> 5;
    const int L = a.L;
    const int off_final = blk0 + (L - 1) * blk1;
    const int off_t = off_final + HP + 4;
    const long long per_tile = 64LL * (KS0 + L * 16 * MT);
    const long long dper_tile = 64LL * (L * 16 * MT);

    {
        const f32x4* src = reinterpret_cast<const f32x4*>(a.packed + off_final);
        for (int i = tid; i < (HP + 4) / 4; i += NT) reinterpret_cast<f32x4*>(s_final)[i] = src[i];
    }
    // image sequence per batch: W_{L-1}^T, ..., W_1^T (tblk1 each), then W_0^T (tblk0)
    constexpr int blkh0 = P.blkh0, blkh1 = P.blkh1;
    const int off_h = off_t + tblk0 + (L - 1) * tblk1;        // scales, then the f16-split forward blocks (lfgc_common.h)
    const int off_img = H16 ? off_h + 32 + LFGC_MAX_LAYERS * HP + HP + blkh0 + (L - 1) * blkh1 : off_t;
    static_assert(lfgc_bwd_offsets_are_the_plans<CH, MT, NF>(1) && lfgc_bwd_offsets_are_the_plans<CH, MT, NF>(LFGC_MAX_LAYERS),
                  "off_final / off_t / off_h / off_img / the tile strides here are not lfgc_make_plan's");
    auto image_src = [&](int l) -> const float* {
        return l == 0 ? a.packed + off_img : a.packed + off_img + tblk0 + (long long)(l - 1) * tblk1;
    };
    if (tid < LFGC_MAX_LAYERS) s_inv[tid] = a.packed[off_h + 8 + tid];      // all LDS lives in the one dynamic array
    lfgc_dma_to_lds(image_src(L - 1), s_ring, (L - 1) == 0 ? tblk0 : tblk1, wave, lane, WAVES);
    __syncthreads();
    unsigned step = 0;
#ifdef LFGC_STAMPS
    unsigned long long bst[8] = {0};
    unsigned long long bst_last = __builtin_amdgcn_s_memtime();
    const unsigned long long bst_t0 = bst_last;
#endif

    constexpr int NPW = H16 ? ((TBMAX / 4 + 63) / 64 + WAVES - 1) / WAVES : 0;   // pieces per wave and image
    LfgcDmaPlan dma = {a.packed, s_ring, tblk1 / 4, __builtin_amdgcn_readfirstlane(wave), (unsigned)lane * 16u, 0ull, 0u};
    const long long N = a.n;
    for (long long batch = blockIdx.x; batch < a.nbatches; batch += gridDim.x) {
        asm volatile("" : "+s"(dma.wave));                // (keeps the pieces' address arithmetic inside the loop)
        // the image of layer l was put in flight one step ago; after the barrier every wave is also done with the
        // other slot, so the next image (layer l-1, or the next batch's first) goes into it
        auto acquire = [&](int l) -> const float* {
            LFGC_BSTAMP(1);                                   // snake' (stash loads) + dstash stores + scale + split
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            LFGC_BSTAMP(2);                                   // wait for stores / DMA + barrier
            const float* img = s_ring + (step & 1) * SLOT;
            const int ln = (l == 0) ? L - 1 : l - 1;
            if (H16) {
                // streamed piece by piece under this step's MFMAs (always a real block: after the last batch the slot is
                // filled once more for nobody, which keeps the MFMA loops free of branches)
                dma.src = image_src(ln);
                dma.dst = s_ring + ((step + 1) & 1) * SLOT;
                dma.nvec = (ln == 0 ? tblk0 : tblk1) / 4;
            } else if (l != 0 || batch + gridDim.x < a.nbatches) {
                lfgc_dma_to_lds(image_src(ln), s_ring + ((step + 1) & 1) * SLOT, ln == 0 ? tblk0 : tblk1, wave, lane, WAVES);
            }
            ++step;
            return img;
        };
        const long long tile_idx = batch * WAVES + wave;
        const long long n = tile_idx * LFGC_TILE_SAMPLES + j;
        const bool valid = n < N;
        const long long nc = valid ? n : (N - 1);
        float dy;
        if constexpr (INPUT_ONLY) dy = valid ? (a.d_out ? a.d_out[n] : 1.0f) : 0.0f;    // no d_out: the gradient of the output itself
        else dy = valid ? a.d_out[n] : 0.0f;
        const float* st_tile = a.stash + tile_idx * per_tile;
        float* dst_tile = a.dstash + tile_idx * dper_tile;

        // ---- final Linear backward: dH_L[k] = Wf[k] * dy -------------------------------------------------
        float dH[16 * MT];
#pragma unroll
        for (int qb = 0; qb < KS1 / 4; ++qb) {
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(s_final + 8 * qb + 4 * hh);
            dH[4 * qb + 0] = w4.x * dy; dH[4 * qb + 1] = w4.y * dy;
            dH[4 * qb + 2] = w4.z * dy; dH[4 * qb + 3] = w4.w * dy;
        }

        // ---- the step at layer l: dA = dH * snake'(a_l), out = W_l^T dA ---------------------------------------------
        // `out`: the row tiles of the product, 16 registers each (their number is the array's); a tile m with !wanted(m)
        // (wave-uniform, and the wanted tiles come first) is not computed and reads as zero.  dA goes to the dstash, and
        // in the f16 builds, scaled by the tile's power of two and split, into the chain; pieces of the next image that
        // no k-step of a computed tile carried go out behind the tiles.
        auto layer_step = [&](int l, auto& out, auto wanted) {
            constexpr int NTILES = sizeof(out) / (16 * sizeof(float));
            float dA[16 * MT];
            lfgc_snake_bwd<MT>(st_tile + 64 * KS0 + (long long)l * P.stash_layer_floats(), dH, dA, lane);
#pragma unroll
            for (int i = 0; i < 16 * MT; ++i) {
                if constexpr (!INPUT_ONLY) dst_tile[(long long)l * P.stash_layer_floats() + i * 64 + lane] = dA[i];
            }
            h16x8 Fhi[2 * MT], Flo[2 * MT];
            float isc = 1.0f;
            if (H16) {
                const float sc = lfgc_tile_pow2_scale<16 * MT>(dA, isc);
                if constexpr (!INPUT_ONLY) { if (lane == 0) a.dscale[tile_idx * L + l] = sc; }
                lfgc_split_scaled<2 * MT, SPLIT>(dA, sc, Fhi, Flo);
            }
            const float* s_row = acquire(l) + j * ST + (H16 ? 8 : 4) * hh;
            const float is = H16 ? s_inv[l] * isc : 1.0f;
            int tiles_done = 0;
#pragma unroll
            for (int m = 0; m < NTILES; ++m) {
                if (wanted(m)) {
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
                    if (H16) acc = lfgc_mfma_tile16<2 * MT, SPLIT, NPW, WAVES>(s_row + 32 * m * ST, Fhi, Flo, acc, &dma, m * 2 * MT);
                    else acc = lfgc_mfma_tile<KS1>(s_row + 32 * m * ST, dA, acc);
#pragma unroll
                    for (int r = 0; r < 16; ++r) out[16 * m + r] = acc[r] * is;
                    ++tiles_done;
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) out[16 * m + r] = 0.0f;
                }
            }
            // (narrow nets: fewer k-steps than pieces, layer 0's image being the larger one; layer 0: few tiles, partly skipped)
            for (int pi = tiles_done * 2 * MT; pi < NPW; ++pi) lfgc_dma_piece<WAVES>(dma, pi);
        };

        LFGC_BSTAMP(0);
        // ---- hidden layers L-1 .. 1 (0-based): every row tile, dH_prev in place of dH ---------------------------------
        for (int l = L - 1; l >= 1; --l) {
            LFGC_BSTAMP(3);                                   // the MFMAs of the layer before (or the head's dH)
            layer_step(l, dH, [](int) { return true; });
        }
        // ---- layer 0: dX0 = W_0^T dA_1 in the forward's input register layout -----------------------------------------
        // scalar-input rows only when d_pos is wanted (wave-uniform); INPUT_ONLY: d_pos is the whole point, every row tile
        float dX[16 * TXA];
        layer_step(0, dX, [&](int m) { return INPUT_ONLY || m < TXF || a.d_pos; });

        LFGC_BSTAMP(3);
        // ---- sampler geometry: the forward's, from the one definition (lfgc_trilinear.h) ---------------------------
        const float* pp = a.pos + 3 * nc;
        const float p0 = pp[0], p1 = pp[1], p2 = pp[2];
        const LfgcAxisCell cx = lfgc_axis_cell(p0, a.W), cy = lfgc_axis_cell(p1, a.H), cz = lfgc_axis_cell(p2, a.D);
        // corner = 4 dz + 2 dy + dx (ATen's order): does it lie in the grid (of a real sample), and where is its (clamped) row
        auto corner_ok = [&](int dx, int dyc, int dz) { return valid && cx.inside(dx) && cy.inside(dyc) && cz.inside(dz); };
        auto corner_off = [&](int dx, int dyc, int dz) {
            return ((long long)(cz.clamped(dz) * a.H + cy.clamped(dyc)) * a.W + cx.clamped(dx)) * a.Cs;
        };

        float gix = 0.0f, giy = 0.0f, giz = 0.0f;
        if constexpr (INPUT_ONLY) {
            // ---- sampler coordinate gradient alone (ATen grid_sampler_3d_backward): the corner loop of the training build
            // below without its staging.  That build's first staging barrier also told every wave that the layer-0 image's
            // slot could be written again; nothing writes it here before the next image does, and that DMA is issued behind
            // the barrier of the NEXT acquire() (the next batch's first layer, or its layer 0 when L == 1), which a wave
            // reaches only after the MFMAs that read this image: the ring's ordinary rule -- the image of step t is
            // overwritten after the barrier of step t + 1 -- now holds across the batch boundary as it does inside a batch.
#pragma unroll
            for (int corner = 0; corner < 8; ++corner) {
                const int dz = corner >> 2, dyc = (corner >> 1) & 1, dx = corner & 1;
                if (corner_ok(dx, dyc, dz))
                    lfgc_corner_coord_grad<CHH>(a.grid + corner_off(dx, dyc, dz) + hh * CHH, dX, dx, dyc, dz, cx.w[dx], cy.w[dyc],
                                                cz.w[dz], gix, giy, giz);
            }
        } else {
            // ---- scatter d feat into d_grid ----------------------------------------------------------------------
            // in-kernel (throughput mode: other waves' work covers the atomics' latency): stage [sample][channel] +
            // per-corner weight / offset in LDS, then one atomic wave-instruction per 64 / CH samples and corner;
            // deferred (a.dfeat; small batches, one wave per SIMD: 128 dependent-latency atomics per wave were 40 % of
            // this kernel): only write the feature gradients out, lfgc_bwd_scatter_kernel scatters them at full occupancy
            const bool stage = a.dfeat == nullptr;            // uniform
            if (stage) __syncthreads();                       // every wave is done with the layer-0 image: reuse its slot
            float* s_df = s_ring + ((step - 1) & 1) * SLOT + wave * SC_WAVE;   // [32][SCS]
            float* s_cw = s_df + 32 * SCS;                    // [32][8] corner weights
            int* s_co = reinterpret_cast<int*>(s_cw + 32 * 8);   // [32][8] corner row offsets (floats)
            static_assert(32 * SCS + 32 * 8 + 32 * 8 == SC_WAVE, "a wave's staging is exactly its share of the slot");
#pragma unroll
            for (int c4 = 0; c4 < CHH / 4; ++c4) {
                f32x4 v;
                v.x = dX[4 * c4 + 0]; v.y = dX[4 * c4 + 1]; v.z = dX[4 * c4 + 2]; v.w = dX[4 * c4 + 3];
                if (stage) *reinterpret_cast<f32x4*>(s_df + j * SCS + hh * CHH + 4 * c4) = v;
                else *reinterpret_cast<f32x4*>(a.dfeat + (tile_idx * 32 + j) * CH + hh * CHH + 4 * c4) = v;
            }
            if (stage || a.d_pos) {
#pragma unroll
            for (int corner = 0; corner < 8; ++corner) {
                const int dz = corner >> 2, dyc = (corner >> 1) & 1, dx = corner & 1;
                const bool ok = corner_ok(dx, dyc, dz);
                const long long off = corner_off(dx, dyc, dz);
                const float w = ok ? __fmul_rn(__fmul_rn(cx.w[dx], cy.w[dyc]), cz.w[dz]) : 0.0f;
                if (stage) { if (hh == 0) s_cw[j * 8 + corner] = w; else s_co[j * 8 + corner] = (int)off; }
                if (a.d_pos && ok)
                    lfgc_corner_coord_grad<CHH>(a.grid + off + hh * CHH, dX, dx, dyc, dz, cx.w[dx], cy.w[dyc], cz.w[dz],
                                                gix, giy, giz);
            }
            }
            if (stage) {
                __syncthreads();                              // staging visible to every lane that reads it
                const int sp = lane / CH, c = lane % CH;
                if (sp < SPI) {
                    for (int i = 0; i < (32 + SPI - 1) / SPI; ++i) {
                        const int smp = i * SPI + sp;
                        if (smp < 32) {
                            const float v = s_df[smp * SCS + c];
#pragma unroll
                            for (int corner = 0; corner < 8; ++corner) {
                                const float w = s_cw[smp * 8 + corner];
                                if (w != 0.0f) atomicAdd(a.d_grid + s_co[smp * 8 + corner] + c, v * w);
                            }
                        }
                    }
                }
            }
        }

        LFGC_BSTAMP(4);                                       // geometry + staging + atomic scatter
        // ---- d_pos = direct columns + Fourier embedding + sampler coordinate gradient ---------------------------
        if (a.d_pos) {
            float sk[NF > 0 ? NF : 1][3], ck[NF > 0 ? NF : 1][3];
            lfgc_fourier_trig<NF>(p0, p1, p2, sk, ck);
            // this lane holds d e[hh*EPH + t] in dX[CHH + t]; evaluate both static mappings, keep this half's
            float dlo[3] = {0.0f, 0.0f, 0.0f}, dhi[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < EPH; ++t) {
                const float d = dX[CHH + t];
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int e = half * EPH + t;
                    float* acc3 = half ? dhi : dlo;
                    if (e < 3) {
                        acc3[e] += d;
                    } else if (e < E) {
                        const int k = (e - 3) / 6, wch = (e - 3) % 6;
                        const float f = lfgc_freq(k);
                        if (wch < 3) acc3[wch] += d * f * ck[k][wch];
                        else acc3[wch - 3] -= d * f * sk[k][wch - 3];
                    }
                }
            }
            float g0 = (hh ? dhi[0] : dlo[0]) + gix * (0.5f * (float)a.W);
            float g1 = (hh ? dhi[1] : dlo[1]) + giy * (0.5f * (float)a.H);
            float g2 = (hh ? dhi[2] : dlo[2]) + giz * (0.5f * (float)a.D);
            g0 += __shfl_xor(g0, 32); g1 += __shfl_xor(g1, 32); g2 += __shfl_xor(g2, 32);
            if (valid && hh == 0) {
                a.d_pos[3 * n + 0] = g0; a.d_pos[3 * n + 1] = g1; a.d_pos[3 * n + 2] = g2;
            }
        }
        LFGC_BSTAMP(5);                                       // d_pos
    }
    // the stream's last image (fetched for nobody) must have landed before the workgroup gives its LDS back
    if (NPW > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef LFGC_STAMPS
    if (a.stamps && lane == 0) {
        unsigned long long* dst = a.stamps + ((long long)blockIdx.x * WAVES + wave) * 20;
        for (int k = 0; k < 8; ++k) dst[k] = bst[k];
        dst[16] = __builtin_amdgcn_s_memtime() - bst_t0;
    }
#endif
}

// Deferred scatter of the feature gradients (small batches): d_grid[corner rows of sample n] += w_corner * dfeat[n].
// A wave takes 8 samples, 64 / CH at a time (one atomic wave-instruction = that many whole channel rows), every lane
// forming its sample's corner weights and offsets itself with the forward's arithmetic (lfgc_trilinear.h); thousands of
// waves, so the float atomics' latency (a cold line per row) is covered by occupancy instead of being waited for 128 times
// in a row.  The walk is shared by the float and the fixed-point scatter: add(i, v, w) accumulates v w into element i.
template <int CH, class ADD>
__device__ __forceinline__ void lfgc_scatter_walk(const float* __restrict__ pos, const float* __restrict__ dfeat, long long n,
                                                  int D, int H, int W, int Cs, ADD add) {
    constexpr int SPI = 64 / CH;                          // samples per wave-instruction
    const int lane = threadIdx.x & 63;
    const long long gw = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int sp = lane / CH, c = lane % CH;
    if (sp >= SPI) return;
#pragma unroll 1
    for (int i = 0; i < 8 / SPI + (8 % SPI != 0); ++i) {
        const long long smp = gw * 8 + i * SPI + sp;
        if (i * SPI + sp >= 8 || smp >= n) continue;
        const float p0 = pos[3 * smp], p1 = pos[3 * smp + 1], p2 = pos[3 * smp + 2];
        const LfgcAxisCell cx = lfgc_axis_cell(p0, W), cy = lfgc_axis_cell(p1, H), cz = lfgc_axis_cell(p2, D);
        const float v = dfeat[smp * CH + c];
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const int dz = corner >> 2, dy = (corner >> 1) & 1, dx = corner & 1;
            const bool ok = cx.inside(dx) && cy.inside(dy) && cz.inside(dz);
            const float w = __fmul_rn(__fmul_rn(cx.w[dx], cy.w[dy]), cz.w[dz]);
            if (ok && w != 0.0f) add(((long long)((cz.i0 + dz) * H + (cy.i0 + dy)) * W + (cx.i0 + dx)) * Cs + c, v, w);
        }
    }
}

template <int CH>
__global__ __launch_bounds__(256) void lfgc_bwd_scatter_kernel(const float* __restrict__ pos, const float* __restrict__ dfeat,
                                                              float* __restrict__ d_grid, long long n, int D, int H, int W, int Cs) {
    lfgc_scatter_walk<CH>(pos, dfeat, n, D, H, W, Cs, [&](long long i, float v, float w) { atomicAdd(d_grid + i, v * w); });
}

// The fixed-point scatter's walk (lfgc_backward.h has the scheme and the passes around this one).
template <int CH>
__global__ __launch_bounds__(256) void lfgc_bwd_scatter_det_kernel(const float* __restrict__ pos, const float* __restrict__ dfeat,
                                                                  long long* __restrict__ acc, const unsigned* __restrict__ maxw,
                                                                  long long n, int D, int H, int W, int Cs) {
    const unsigned mb = *maxw;
    if (mb == 0u || mb >= kLfgcDetNonFinite) return;                   // nothing to add / the finish pass writes NaN
    const double inv_q = lfgc_det_pow2(-lfgc_det_qexp(mb, n));
    lfgc_scatter_walk<CH>(pos, dfeat, n, D, H, W, Cs, [&](long long i, float v, float w) {
        const long long k = __double2ll_rn((double)__fmul_rn(v, w) * inv_q);        // |k| <= 2^B: |v| <= max, w <= 1
        atomicAdd(reinterpret_cast<unsigned long long*>(acc + i), (unsigned long long)k);
    });
}

template <int CH, int MT, int NF, int WAVES, int PREC, bool INPUT_ONLY>
static int lfgc_launch_bwd_data(const LfgcBwdArgs& a, int lds_bytes, int grid_data, hipStream_t stream) {
    return lfgc_launch<lfgc_bwd_data_kernel<CH, MT, NF, WAVES, PREC, INPUT_ONLY>>(dim3(grid_data), dim3(WAVES * 64), lds_bytes,
                                                                                  stream, a);
}

// The data kernel's build for (waves, h16): waves = waves per workgroup (4 or 8, chosen by the caller together with
// a.nbatches), h16 = the C-ABI precision code: 0 exact f32 MFMA chain, 1 f16 hi/lo split, 2 single f16 product.
template <int CH, int MT, int NF, bool INPUT_ONLY>
static int lfgc_launch_bwd_data_any(const LfgcBwdArgs& a, int waves, int h16, int lds_bytes, int grid_data, hipStream_t stream) {
    if (h16 == 1) return waves == 8 ? lfgc_launch_bwd_data<CH, MT, NF, 8, 1, INPUT_ONLY>(a, lds_bytes, grid_data, stream)
                                    : lfgc_launch_bwd_data<CH, MT, NF, 4, 1, INPUT_ONLY>(a, lds_bytes, grid_data, stream);
    if (h16 == 2) return waves == 8 ? lfgc_launch_bwd_data<CH, MT, NF, 8, 2, INPUT_ONLY>(a, lds_bytes, grid_data, stream)
                                    : lfgc_launch_bwd_data<CH, MT, NF, 4, 2, INPUT_ONLY>(a, lds_bytes, grid_data, stream);
    return waves == 8 ? lfgc_launch_bwd_data<CH, MT, NF, 8, 0, INPUT_ONLY>(a, lds_bytes, grid_data, stream)
                      : lfgc_launch_bwd_data<CH, MT, NF, 4, 0, INPUT_ONLY>(a, lds_bytes, grid_data, stream);
}
