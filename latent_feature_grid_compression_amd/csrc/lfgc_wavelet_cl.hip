// lfgc_wavelet_cl.hip -- the LAST wavelet level with the dense grid in the sampler's channel-last layout (gfx950).
//   lfgc_idwt_level_cl_f32      wavelet_transform/Torch_Wavelet_Transform.py:91-104 (+ crop :69-73) writing (t0,t1,t2,Cs)
//   lfgc_idwt_level_cl_bwd_f32  its adjoint reading the gradient of that (t0,t1,t2,Cs) grid
//   lfgc_idwt_level_cl_drop_len_f32 / _bwd_len_f32  the same two with the pruning layers' per-coefficient factors (and
//                               the penalty gradients) folded in: the DROP builds of both kernels, same contract as the
//                               channel-first lfgc_idwt_level_drop_len_f32 / _bwd_len_f32 (lfgc_wavelet.hip)
// so that decode_volume() needs no layout conversion pass (lfgc_grid_layout_f32) on either direction, with or without
// drop layers.  Separable filter banks only (`taps`); the dense-stencil path keeps the channel-first kernels + the
// conversion.  The non-DROP instantiations are unchanged by the DROP template parameter (every new field and statement
// sits behind `if (DROP)`; same instruction streams, same registers, same LDS).
//
// Templates on the half filter length K: K = 2 (db2) and K = 1 (Haar, no neighbour cells and no z carry: each 2x2x2
// output block is a butterfly of one cell's 8 bands).  Longer filters take the channel-first kernels + the conversion.
//
// Both kernels have one shape.  A workgroup owns 32 consecutive cells of the flattened (y,x) plane, a group of CW = 32,
// 16 or 8 channels (CW / 2 waves), and walks a chunk of z steps.  The coefficient side is channel-first (contiguous along the cells), the
// grid side channel-last (contiguous along the channels), so the arithmetic runs with the lanes along whichever side is
// being READ -- straight from global memory, neighbouring lanes on neighbouring addresses, the 4x reuse between
// neighbouring cells served by L1/L2 -- and the 8 results per (cell, channel) go through an LDS tile that is read back
// with the lanes along the other side: every global store instruction writes whole 64/128-byte runs.  The tile is double
// buffered: one barrier per z step; the stores of step s and the loads of step s+1 are in flight under the arithmetic
// (a thread holds exactly one step's 32 input values; the next step's loads are issued as soon as they are contracted).
// Along z the stencil slides: a coefficient plane (synthesis) / a pair of source planes (adjoint) is read and contracted
// in-plane ONCE; what it contributes to the following step is carried in 8 registers per (cell, channel).
// Work items (plane tile, channel group, z chunk) are dealt to the XCDs so that the two channel groups of a tile (they
// write the two halves of the same 128-byte lines) and neighbouring tiles (they share coefficient rows / source voxels)
// run on the same XCD and meet in its L2.
#include "lfgc_common.h"
#include "lfgc_drop_value.h"   // drop_value(), sign_of()
#include <cstdlib>

namespace {

constexpr int kCells = 32;           // plane cells per workgroup

template <int CW> struct ClShape {   // CW: channels per workgroup (8, 16; synthesis also 32)
    static constexpr int NW = CW / 2;                    // waves per workgroup
    static constexpr int CPW = 64 / CW;                  // voxels / cells per wave instruction with the lanes along channels
    static constexpr int VOX = CW + 1;                   // synthesis tile [8 parities][32 cells][CW + 1]
    static constexpr int CHS = 8 * kCells + 1;           // adjoint tile [CW channels][8 bands][32 cells] + 1
};

// Loads go through buffer descriptors: a 32-bit lane offset on a wave-uniform (descriptor, scalar offset) pair costs one
// VGPR per distinct lane offset instead of a 64-bit address per load, and a lane offset >= num_records reads as 0.0 --
// taps outside the level (the conv_transpose3d / F.pad zeros) are encoded as kOutside in the lane offset: no select per
// value, no address clamp.  The scalar offset is not part of the range check, so it may be any in-range plane offset.
// A thread holds one step's 32 input values; the next step's are requested as soon as these are contracted and fly
// under the rest of the step (the carry arithmetic, the tile, the barrier, the stores).  Requesting them a whole step
// ahead (two register sets, each path through a step with its own wait counts) was built and measured: same time at
// 114 instead of 96 VGPRs (synthesis), slower where it cost a workgroup per CU (adjoint: 146 VGPRs) -- the kernels
// are not latency-bound.
constexpr unsigned kOutside = 0x40000000u;            // arrays on these paths are < 2^30 bytes (host check)
typedef __amdgpu_buffer_rsrc_t cl_srd;
#ifndef LFGC_CL_ABLATE
#define LFGC_CL_ABLATE 0             // diagnostics (tools/ab_wavelet_cl.py): 1 no global stores, 2 no global loads
#endif

__device__ __forceinline__ cl_srd cl_make_srd(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ void cl_load(float& dst, cl_srd r, unsigned lane_off, unsigned uniform_off) {
    if (LFGC_CL_ABLATE & 2) { dst = __builtin_bit_cast(float, (lane_off ^ uniform_off) & 0x3fffffu); return; }
    dst = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)lane_off, (int)uniform_off, 0));
}

// NT: non-temporal (streaming) store.  The synthesis writes whole 64/128-byte runs of a grid nobody reads before the
// kernel ends; keeping them out of the L2 leaves it to the coefficient lines that neighbouring workgroups share
// (measured, cfg-5 last level: 205 -> 180 us; only with whole lines, i.e. 32-channel workgroups: 64- and 32-byte
// pieces get slower).  Only for grids that could not stay in the 32 MB of L2 anyway: the cfg-3 grid (32 MiB) is sampled
// right after the decode and the train step is 4 us faster with it cached (0.405 vs 0.409 ms).  The adjoint's stores
// are 128-byte pieces of unaligned runs that complete each other's lines in the L2: streaming them costs (192 ->
// 236 us), and so does streaming any of the loads.
template <bool NT>
__device__ __forceinline__ void cl_store(float v, cl_srd r, unsigned lane_off, unsigned uniform_off) {
    if ((LFGC_CL_ABLATE & 1) && v != 1.2345e-30f) return;
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), r, (int)lane_off, (int)uniform_off, NT ? 2 : 0);   // lane_off >= num_records: dropped
}

// Workgroup b works on item (b % 8) * ceil(total / 8) + b / 8 (workgroups are dealt round-robin to the 8 XCDs);
// item = (z chunk * ptiles + plane tile) * ngroups + channel group.
__device__ __forceinline__ bool cl_work_item(int ptiles, int ngroups, int nchunks, int* pt, int* cg, int* zc) {
    const int total = ptiles * ngroups * nchunks;
    const int per = (total + 7) >> 3;
    const int item = (int)(blockIdx.x & 7u) * per + (int)(blockIdx.x >> 3);
    if ((int)(blockIdx.x >> 3) >= per || item >= total) return false;
    const int tile = item / ngroups;
    *cg = item - tile * ngroups;
    *zc = tile / ptiles;
    *pt = tile - *zc * ptiles;
    return true;
}

template <int K>
struct IdwtClArgs {
    const float* lll;   // (C, d0,d1,d2)
    const float* hf;    // (C, 7, d0,d1,d2)
    float* out;         // (t0,t1,t2, cs)
    int C, cs, d0, d1, d2, t0, t1, t2, o0, o1, o2;   // o = crop offset floor((2d+2K-2-t)/2)
    int zchunk, ptiles, ngroups, nchunks;
    float taps[4 * K];  // [low | high][tap]
    // DROP build only: the pruning layers' per-coefficient factors, shared by all channels (lfgc_wavelet.hip: IdwtArgs)
    const float* mul_l; // (d0,d1,d2) or NULL
    const float* mul_h; // (7, d0,d1,d2) or NULL
    float thr_l, thr_h; // NaN: value = x * m;  else the masked straight-through rule (drop_value)
};

// Synthesis: out_full[o] = sum_{s,t} in[s][i] F_s[t], o = 2 i + t per axis; cell j = (jz,jy,jx) in [0,d+K-2] per axis
// produces the 2x2x2 outputs o = 2 j + p from the coefficient cells i = j - e (e in [0,K)) with taps t = p + 2 e.
// Plane iz of the coefficients is contracted over x and y once (Y[sz][py][px]); its e_z = 0 part completes cell slice
// jz = iz (added to the carry of the earlier planes), its e_z = e part is carried to slice iz + e.
// Arithmetic role: 32 cells x 2 channels per wave: channel = c0 + 2 wave + lane / 32.
// DROP: every coefficient passes through its drop layer (drop_value) before the in-plane contraction.  Its factor sits
// at the same cell of a (d0,d1,d2) / (7,d0,d1,d2) array without the channel, so all CW channels of the workgroup use the
// same 8 K^2 x 32 factors of a plane: the workgroup fetches them ONCE (1 to 4 per thread, the same neighbour-cell offsets
// through descriptors of the factor arrays, kOutside neighbours read 0 like their coefficients), a step ahead, into a
// double-buffered LDS table [neighbour][band][cell] that the arithmetic role reads back with its lanes along the cells.
// Holding a thread's 8 K^2 factors in registers next to its coefficients instead was built first: 164 VGPRs for K = 2
// (3 waves per SIMD; 67 spilled in the 16-wave workgroup, which is capped at 128).
template <int CW, int CELLS, bool NT, int K, bool DROP>
__global__ __launch_bounds__(CW * CELLS) void idwt_cl_kernel(const IdwtClArgs<K> a) {
    constexpr int L = 2 * K;
    constexpr int KC = K > 1 ? K - 1 : 1;             // z-carry slots (8 floats each)
    constexpr int CPL = 64 / CELLS;                   // channels per wave in the arithmetic role
    constexpr int CPW = ClShape<CW>::CPW, VOX = ClShape<CW>::VOX;
    constexpr int TILE = 8 * CELLS * VOX;
    extern __shared__ __attribute__((aligned(16))) float s_tile[];      // [2][TILE]
    int pt, cg, zc;
    if (!cl_work_item(a.ptiles, a.ngroups, a.nchunks, &pt, &cg, &zc)) return;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n0 = a.d0 + (K - 1), n1 = a.d1 + (K - 1), n2 = a.d2 + (K - 1);
    const int plane_cells = n1 * n2;
    const int f0 = pt * CELLS;
    const int c0 = cg * CW;
    const int jz_begin = zc * a.zchunk, jz_end = min(jz_begin + a.zchunk, n0);
    const int dplane = a.d1 * a.d2;
    const int dvol = dplane * a.d0;                   // C * 7 * dvol * 4 < 2^30 (host check)

    // arithmetic role: byte offsets of the K*K neighbour cells (jy - ey, jx - ex) inside a coefficient plane, plus the
    // lane's channel parity; everything else of the address is wave-uniform
    const int cell = lane & (CELLS - 1), chalf = lane / CELLS;
    const int cw = CPL * w + chalf;                      // channel within the group
    unsigned offl[K * K];                              // low band; the detail bands' offset is offl + hshift (7 bands per channel)
    unsigned hshift;
    {
        const int f = f0 + cell;
        const int fc = min(f, plane_cells - 1);
        const int jy = fc / n2, jx = fc - jy * n2;
#pragma unroll
        for (int q = 0; q < K * K; ++q) {
            const int cy = jy - q / K, cx = jx - q % K;
            const bool ok = f < plane_cells && c0 + cw < a.C && cy >= 0 && cy < a.d1 && cx >= 0 && cx < a.d2;
            offl[q] = ok ? 4u * (unsigned)(chalf * dvol + cy * a.d2 + cx) : kOutside;
        }
        hshift = 4u * (unsigned)(chalf * 6 * dvol);        // kOutside + hshift stays >= num_records: 6 * dvol * 4 < 2^30
    }
    const cl_srd rl = cl_make_srd(a.lll, (unsigned)(a.C * dvol * 4));
    const cl_srd rh = cl_make_srd(a.hf, (unsigned)(a.C * 7 * dvol * 4));
    const bool wave_live = c0 + CPL * w < a.C;           // wave-uniform: this wave's channel pair exists

    // store role: lanes = CW channels x CPW voxels; this wave's cells are [CPW w, CPW w + CPW), instruction p = parity:
    // one cell per thread
    const int fch = lane & (CW - 1), fcell = w * CPW + lane / CW;
    unsigned vo[4];                                    // byte offset of output (py,px) of the cell in a z slice; kOutside when cropped away
    {
        const int f = f0 + fcell;
        const int fc = min(f, plane_cells - 1);
        const int jy = fc / n2, jx = fc - jy * n2;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int oy = 2 * jy + (p >> 1) - a.o1, ox = 2 * jx + (p & 1) - a.o2;
            const bool ok = f < plane_cells && c0 + fch < a.cs && oy >= 0 && oy < a.t1 && ox >= 0 && ox < a.t2;
            vo[p] = ok ? 4u * (unsigned)((oy * a.t2 + ox) * a.cs + c0 + fch) : kOutside;
        }
    }
    const bool pad_channel = c0 + fch >= a.C;
    const int slice = a.t1 * a.t2 * a.cs;
    const cl_srd rout = cl_make_srd(a.out, (unsigned)(a.t0 * slice * 4));

    // DROP, factor role: table element e = (q * 8 + band) * CELLS + cell, elements thread + k * (workgroup size).  The
    // band is part of the lane offset (it differs inside a wave), so each element is asked of both factor arrays with
    // the one it does not belong to (or that is NULL) marked kOutside: reads 0, and the two results are OR-ed.
    constexpr int NF = 8 * K * K * CELLS;              // factors of one coefficient plane
    constexpr int FPT = DROP ? (NF + CW * CELLS - 1) / (CW * CELLS) : 1;
    float* s_fac = s_tile + 2 * TILE;                  // [2][NF], slot = plane & 1
    unsigned fol[FPT], foh[FPT];
    float fv[FPT];
    cl_srd rml, rmh;
    if (DROP) {
        rml = cl_make_srd(a.mul_l, a.mul_l ? (unsigned)(dvol * 4) : 0u);
        rmh = cl_make_srd(a.mul_h, a.mul_h ? (unsigned)(7 * dvol * 4) : 0u);
#pragma unroll
        for (int k = 0; k < FPT; ++k) {
            const int e = (int)threadIdx.x + k * CW * CELLS;
            const int q = (e / CELLS) >> 3, sb = (e / CELLS) & 7;
            const int f = f0 + e % CELLS;
            const int fc = min(f, plane_cells - 1);
            const int jy = fc / n2, jx = fc - jy * n2;
            const int cy = jy - q / K, cx = jx - q % K;
            const bool ok = e < NF && f < plane_cells && cy >= 0 && cy < a.d1 && cx >= 0 && cx < a.d2;
            fol[k] = ok && sb == 0 && a.mul_l ? 4u * (unsigned)(cy * a.d2 + cx) : kOutside;
            foh[k] = ok && sb > 0 && a.mul_h ? 4u * (unsigned)((sb - 1) * dvol + cy * a.d2 + cx) : kOutside;
        }
    }
    auto fac_issue = [&](int pz) {                     // factors of coefficient plane pz -> fv
#pragma unroll
        for (int k = 0; k < FPT; ++k) {
            float l, h;
            cl_load(l, rml, fol[k], 4u * (unsigned)(pz * dplane));
            cl_load(h, rmh, foh[k], 4u * (unsigned)(pz * dplane));
            fv[k] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, l) | __builtin_bit_cast(unsigned, h));
        }
    };
    auto fac_put = [&](int pz) {                       // fv -> table slot of plane pz
#pragma unroll
        for (int k = 0; k < FPT; ++k) {
            const int e = (int)threadIdx.x + k * CW * CELLS;
            if (e < NF) s_fac[(pz & 1) * NF + e] = fv[k];
        }
    };

    float R[8 * K * K];                                // [neighbour q][band]
    float carry[8 * KC];                               // [slice iz + 1 + e][parity]
#pragma unroll
    for (int p = 0; p < 8 * KC; ++p) carry[p] = 0.0f;

    auto issue = [&](int iz) {                         // coefficient plane iz: K*K neighbour cells x 8 bands of this lane's channel
        const unsigned sl = 4u * (unsigned)((c0 + CPL * w) * dvol + iz * dplane);
#pragma unroll
        for (int q = 0; q < K * K; ++q) cl_load(R[q * 8], rl, offl[q], sl);
#pragma unroll
        for (int sb = 1; sb < 8; ++sb) {
            const unsigned sh = 4u * (unsigned)(((c0 + CPL * w) * 7 + sb - 1) * dvol + iz * dplane);
#pragma unroll
            for (int q = 0; q < K * K; ++q) cl_load(R[q * 8 + sb], rh, offl[q] + hshift, sh);
        }
    };

    int iz = jz_begin - (K - 1);
    if (wave_live && iz >= 0) issue(iz);
    if (DROP) {
        // The table of plane p is filled during step p - 1, before that step's barrier (DROP: every step has one): its
        // slot was last read in step p - 2, which every wave left through that step's barrier.  First plane: here.
        if (iz >= 0) { fac_issue(iz); fac_put(iz); }
        __syncthreads();
    }
    int buf = 0;
#pragma unroll 1
    for (; iz < jz_end; ++iz) {
        const bool emit = iz >= jz_begin;
        const bool plane_ok = iz >= 0 && iz < a.d0;
        const bool next_ok = iz + 1 < jz_end && iz + 1 < a.d0;
        float* tile = s_tile + buf * TILE;
        if (DROP && next_ok) fac_issue(iz + 1);                   // every wave, also one without channels
        if (wave_live) {
            float outv[8];
            if (plane_ok) {
                if (DROP) {
                    const float* fac = s_fac + (iz & 1) * NF + cell;
                    if (a.mul_l) {
#pragma unroll
                        for (int q = 0; q < K * K; ++q) R[q * 8] = drop_value(R[q * 8], fac[q * 8 * CELLS], a.thr_l, a.thr_l == a.thr_l);
                    }
                    if (a.mul_h) {
#pragma unroll
                        for (int q = 0; q < K * K; ++q)
#pragma unroll
                            for (int sb = 1; sb < 8; ++sb)
                                R[q * 8 + sb] = drop_value(R[q * 8 + sb], fac[(q * 8 + sb) * CELLS], a.thr_h, a.thr_h == a.thr_h);
                    }
                }
                float X[K][2][2][2];                              // [ey][sz][sy][px]
#pragma unroll
                for (int q = 0; q < 4 * K; ++q) {
                    const int ey = q >> 2, sz = (q >> 1) & 1, sy = q & 1;
#pragma unroll
                    for (int px = 0; px < 2; ++px) {
                        float t = 0.0f;
#pragma unroll
                        for (int ex = 0; ex < K; ++ex)
#pragma unroll
                            for (int sx = 0; sx < 2; ++sx)
                                t = __builtin_fmaf(R[(ey * K + ex) * 8 + sz * 4 + sy * 2 + sx], a.taps[sx * L + px + 2 * ex], t);
                        X[ey][sz][sy][px] = t;
                    }
                }
                if (next_ok) issue(iz + 1);                       // R is free: the next plane flies under the rest of the step
                float Y[2][2][2];                                 // [sz][py][px]
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int sz = q >> 2, py = (q >> 1) & 1, px = q & 1;
                    float t = 0.0f;
#pragma unroll
                    for (int ey = 0; ey < K; ++ey)
#pragma unroll
                        for (int sy = 0; sy < 2; ++sy)
                            t = __builtin_fmaf(X[ey][sz][sy][px], a.taps[sy * L + py + 2 * ey], t);
                    Y[sz][py][px] = t;
                }
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const int pz = p >> 2, py = (p >> 1) & 1, px = p & 1;
                    float t = K > 1 ? carry[p] : 0.0f;            // planes iz - e (e_z = e >= 1)
                    float n[KC];                                  // slices iz + e, e = 1 .. K-1
#pragma unroll
                    for (int e = 1; e < K; ++e) n[e - 1] = e < K - 1 ? carry[e * 8 + p] : 0.0f;
#pragma unroll
                    for (int sz = 0; sz < 2; ++sz) {
                        t = __builtin_fmaf(Y[sz][py][px], a.taps[sz * L + pz], t);
#pragma unroll
                        for (int e = 1; e < K; ++e) n[e - 1] = __builtin_fmaf(Y[sz][py][px], a.taps[sz * L + pz + 2 * e], n[e - 1]);
                    }
                    outv[p] = t;
#pragma unroll
                    for (int e = 1; e < K; ++e) carry[(e - 1) * 8 + p] = n[e - 1];
                }
            } else {
                if (next_ok) issue(iz + 1);
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    outv[p] = K > 1 ? carry[p] : 0.0f;
#pragma unroll
                    for (int e = 1; e < K; ++e) carry[(e - 1) * 8 + p] = e < K - 1 ? carry[e * 8 + p] : 0.0f;
                }
            }
            if (emit) {
#pragma unroll
                for (int p = 0; p < 8; ++p) tile[(p * CELLS + cell) * VOX + cw] = outv[p];
            }
        }
        if (DROP) {
            if (next_ok) fac_put(iz + 1);
            if (!emit) __syncthreads();
        }
        if (emit) {
            __syncthreads();
            // one barrier per step is enough: the other buffer is written only after the NEXT barrier, which every wave
            // reaches after it has finished reading this one's predecessor
#pragma unroll
            for (int pz = 0; pz < 2; ++pz) {
                const int oz = 2 * iz + pz - a.o0;
                if (oz >= 0 && oz < a.t0) {
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const float v = tile[((pz * 4 + p) * CELLS + fcell) * VOX + fch];
                        cl_store<NT>(pad_channel ? 0.0f : v, rout, vo[p], 4u * (unsigned)(oz * slice));
                    }
                }
            }
            buf ^= 1;
        }
    }
}

template <int K>
struct AnalysisClArgs {
    const float* src;      // (n0,n1,n2, cs)
    float* band0;          // band 0 of channel c at band0 + c * dvol
    float* bandh;          // band s >= 1 of channel c at bandh + (c * 7 + s - 1) * dvol
    int C, cs, n0, n1, n2, lo0, lo1, lo2, d0, d1, d2;
    int zchunk, ptiles, ngroups, nchunks;
    float taps[4 * K];
    // DROP build only (lfgc_wavelet.hip: AnalysisArgs)
    const float* lll;      // forward inputs (C, d0,d1,d2), (C, 7, d0,d1,d2): needed for d_mul and the L2 penalty
    const float* hf;
    const float* mul_l;    // (d0,d1,d2) or NULL
    const float* mul_h;    // (7, d0,d1,d2) or NULL
    float* d_mul_l;        // (d0,d1,d2) or NULL, pre-zeroed
    float* d_mul_h;        // (7, d0,d1,d2) or NULL, pre-zeroed
    const float* g_l2_l; const float* g_l2_h; const float* g_l1_l; const float* g_l1_h;   // penalty gradients folded in
    int dmul_gstride;      // 0: every channel group adds into the one d_mul_* array; else group cg adds into its own slice
                           // d_mul_* + cg * dmul_gstride (floats): one add onto zero per address, exact in any order
};

// Adjoint: band_s[c][i] = sum_t src[2 i + t - lo][c] F_s[t].  Step iz reads the source planes 2 iz - lo0 + L-2 + {0, 1},
// contracts each over x and y (P[sy][sx]) and combines them with the L - 2 planes carried from the earlier steps.
// Arithmetic role: lanes = CW channels x CPW cells; cell = wave * CPW + lane / CW.
// DROP (the contract of analysis_kernel<true, ...>, lfgc_wavelet.hip): stored gradient = band_s m_s (+ 2 g coef_s for an
// L2 penalty), d_m_s[i] += sum_c band_s[c][i] coef_s[c][i] (+ g sign(m) for an L1 penalty, once per address: channel
// group 0).  In the store role a lane's store address into d_lll / d_hf is the address of the matching lll / hf value
// (same layout): coef is loaded there, coalesced, the factor at the same cell without the channel.  The lane puts
// band coef back into its tile slot; after a second barrier the workgroup sums the CW channels of every (band, cell) in
// LDS and issues ONE float atomic per (band, cell) -- whole runs of consecutive cells per wave instruction -- instead of
// one per channel.
template <int CW, int NG, int K, bool DROP>   // NG: cell groups of 32 per workgroup (the channel-first runs it writes are 128 NG bytes)
__global__ __launch_bounds__(32 * CW) void analysis_cl_kernel(const AnalysisClArgs<K> a) {
    constexpr int L = 2 * K;
    constexpr int CT = L > 2 ? L - 2 : 1;             // carried source planes
    constexpr int CPW = ClShape<CW>::CPW, CELLS = kCells * NG, CHS = 8 * CELLS + 1;
    constexpr int TILE = CW * CHS;
    extern __shared__ __attribute__((aligned(16))) float s_tile[];      // [2][TILE]: [channel][band][cell] + 1
    int pt, cg, zc;
    if (!cl_work_item(a.ptiles, a.ngroups, a.nchunks, &pt, &cg, &zc)) return;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int plane_cells = a.d1 * a.d2;
    const int f0 = pt * CELLS;
    const int c0 = cg * CW;
    const int iz_begin = zc * a.zchunk, iz_end = min(iz_begin + a.zchunk, a.d0);
    const int dvol = plane_cells * a.d0;              // C * 7 * dvol * 4 < 2^30 (host check)
    const int nplane = a.n1 * a.n2 * a.cs;            // n0 * nplane * 4 < 2^30 (host check)

    // arithmetic role: lanes = CW channels x CPW cells; cell of group g = 32 g + wave * CPW + lane / CW
    const int ch = lane & (CW - 1), cslot = w * CPW + lane / CW;
    unsigned ro[NG][L], co[NG][L]; // byte offsets of row ty / column tx (+ channel) inside a source plane; kOutside when outside
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int f = f0 + g * kCells + cslot;
        const bool live = f < plane_cells && c0 + ch < a.C;
        const int fc = min(f, plane_cells - 1);
        const int iy = fc / a.d2, ix = fc - iy * a.d2;
#pragma unroll
        for (int t = 0; t < L; ++t) {
            const int uy = 2 * iy + t - a.lo1, ux = 2 * ix + t - a.lo2;
            ro[g][t] = (live && uy >= 0 && uy < a.n1) ? 4u * (unsigned)(uy * a.n2 * a.cs) : kOutside;
            co[g][t] = (ux >= 0 && ux < a.n2) ? 4u * (unsigned)(ux * a.cs + c0 + ch) : kOutside;
        }
    }
    const cl_srd rs = cl_make_srd(a.src, (unsigned)(a.n0 * nplane * 4));

    // store role: NG == 1: lane = (cell, channel parity), one instruction per band; NG >= 2: lane = cell, one instruction per
    // band, channel and 64 cells
    unsigned so0, soh;
    unsigned som = 0;              // DROP: the cell inside a factor plane (no channel part)
    if (NG == 1) {
        const int sf = f0 + (lane & 31), half = lane >> 5;
        const bool ok = sf < plane_cells && c0 + 2 * w + half < a.C;
        so0 = ok ? 4u * (unsigned)(half * dvol + sf) : kOutside;
        soh = ok ? 4u * (unsigned)(half * 7 * dvol + sf) : kOutside;
        if (DROP) som = ok ? 4u * (unsigned)sf : kOutside;
    } else {
        so0 = soh = 4u * (unsigned)(f0 + lane);
        if (DROP) som = so0;
    }
    const cl_srd rb0 = cl_make_srd(a.band0, (unsigned)(a.C * dvol * 4));
    const cl_srd rbh = cl_make_srd(a.bandh, (unsigned)(a.C * 7 * dvol * 4));
    // DROP: descriptors of the coefficients and the factors; an operand that is absent (or, coefficients, not needed: no
    // factor gradient and no L2 penalty) gets an EMPTY one: its loads stay in the instruction stream, read 0.0 and
    // move no bytes -- the store role below is one branch-free block
    const bool need_l = DROP && a.lll && (a.d_mul_l || a.g_l2_l), need_h = DROP && a.hf && (a.d_mul_h || a.g_l2_h);
    const cl_srd rc0 = cl_make_srd(DROP ? a.lll : nullptr, need_l ? (unsigned)(a.C * dvol * 4) : 0u);
    const cl_srd rch = cl_make_srd(DROP ? a.hf : nullptr, need_h ? (unsigned)(a.C * 7 * dvol * 4) : 0u);
    const cl_srd rm0 = cl_make_srd(DROP ? a.mul_l : nullptr, DROP && a.mul_l ? (unsigned)(dvol * 4) : 0u);
    const cl_srd rmh = cl_make_srd(DROP ? a.mul_h : nullptr, DROP && a.mul_h ? (unsigned)(7 * dvol * 4) : 0u);
    // DROP: which operands exist, as bits [low, detail] of one word, and the penalty scalars by value (scalar registers
    // are what these builds run out of: a pointer costs two and stays live for its NULL test)
    enum { kMul = 1, kDMul = 4, kL2 = 16, kL1 = 64 };
    unsigned has = 0;
    float g2l = 0.0f, g2h = 0.0f, g1l = 0.0f, g1h = 0.0f;
    if (DROP) {
        has = (a.mul_l ? kMul : 0) | (a.mul_h ? 2 * kMul : 0) | (a.d_mul_l ? kDMul : 0) | (a.d_mul_h ? 2 * kDMul : 0) |
              (a.g_l2_l ? kL2 : 0) | (a.g_l2_h ? 2 * kL2 : 0) | (a.g_l1_l ? kL1 : 0) | (a.g_l1_h ? 2 * kL1 : 0);
        if (a.g_l2_l) g2l = 2.0f * *a.g_l2_l;
        if (a.g_l2_h) g2h = 2.0f * *a.g_l2_h;
        if (a.g_l1_l) g1l = *a.g_l1_l;
        if (a.g_l1_h) g1h = *a.g_l1_h;
    }
    // DROP, store role: band value v of band sb whose store address is (lo, uo) and whose factor is at (mlo, mo) -> the
    // value to store; the lane's share of the factor gradient goes back into its tile slot (read only where a factor
    // gradient is wanted).  Selects on wave-uniform bits, no branches: the 8 bands' loads are in flight together.
    auto fold = [&](int sb, float v, unsigned lo, unsigned uo, unsigned mlo, unsigned mo, float* slot) -> float {
        const unsigned bit = sb == 0 ? 1u : 2u;
        float x, m;
        cl_load(x, sb == 0 ? rc0 : rch, lo, uo);
        cl_load(m, sb == 0 ? rm0 : rmh, mlo, mo);
        *slot = v * x;
        v = (has & bit * kMul) ? v * m : v;
        return (has & bit * kL2) ? __builtin_fmaf(sb == 0 ? g2l : g2h, x, v) : v;
    };

    float R[2 * L * L];            // [plane k][ty*L+tx] of the cell group in flight
    float carry[NG][CT][4];        // [group][plane tz = 0 .. L-3 of the next step][sy*2+sx]
#pragma unroll
    for (int i = 0; i < 4 * CT * NG; ++i) carry[i / (4 * CT)][(i >> 2) % CT][i & 3] = 0.0f;

    auto plane_in = [&](int iz, int k) { const int uz = 2 * iz - a.lo0 + L - 2 + k; return uz >= 0 && uz < a.n0; };
    auto issue = [&](int iz, int g) {                  // source planes 2 iz - lo0 + L-2 + {0,1} (outside the level: not read, P = 0)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (plane_in(iz, k)) {
                const unsigned sp = 4u * (unsigned)((2 * iz - a.lo0 + L - 2 + k) * nplane);
#pragma unroll
                for (int t = 0; t < L * L; ++t) cl_load(R[k * L * L + t], rs, ro[g][t / L] + co[g][t % L], sp);
            }
        }
    };

    int iz = iz_begin - (K - 1);
    issue(iz, 0);
    int buf = 0;
#pragma unroll 1
    for (; iz < iz_end; ++iz) {
        const bool emit = iz >= iz_begin;
        float* tile = s_tile + buf * TILE;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float P[2][4];                                        // new planes tz = 2, 3: [sy*2+sx]
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (plane_in(iz, k)) {
                    float X[L][2];
#pragma unroll
                    for (int ty = 0; ty < L; ++ty) {
                        float x0 = 0.0f, x1 = 0.0f;
#pragma unroll
                        for (int tx = 0; tx < L; ++tx) {
                            x0 = __builtin_fmaf(R[k * L * L + ty * L + tx], a.taps[tx], x0);
                            x1 = __builtin_fmaf(R[k * L * L + ty * L + tx], a.taps[L + tx], x1);
                        }
                        X[ty][0] = x0; X[ty][1] = x1;
                    }
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4) {
                        float t = 0.0f;
#pragma unroll
                        for (int ty = 0; ty < L; ++ty) t = __builtin_fmaf(X[ty][s4 & 1], a.taps[(s4 >> 1) * L + ty], t);
                        P[k][s4] = t;
                    }
                } else {
#pragma unroll
                    for (int s4 = 0; s4 < 4; ++s4) P[k][s4] = 0.0f;
                }
            }
            // R is free: the next group's / step's planes fly under the rest of this one
            if (g + 1 < NG) issue(iz, g + 1);
            else if (iz + 1 < iz_end) issue(iz + 1, 0);
            if (emit) {
#pragma unroll
                for (int sb = 0; sb < 8; ++sb) {
                    const int s4 = sb & 3, sz = sb >> 2;
                    // source plane tz of this step: carried for tz < L-2, new (P) for the last two
                    auto plane = [&](int tz) { return tz < L - 2 ? carry[g][tz < CT ? tz : 0][s4] : P[tz >= L - 2 ? tz - (L - 2) : 0][s4]; };
                    float t = plane(0) * a.taps[sz * L + 0];
#pragma unroll
                    for (int tz = 1; tz < L; ++tz) t = __builtin_fmaf(plane(tz), a.taps[sz * L + tz], t);
                    tile[ch * CHS + sb * CELLS + g * kCells + cslot] = t;
                }
            }
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
#pragma unroll
                for (int tz = 0; tz + 2 < L - 2; ++tz) carry[g][tz][s4] = carry[g][tz + 2][s4];
                if (L > 2) { carry[g][L > 2 ? L - 4 : 0][s4] = P[0][s4]; carry[g][L > 2 ? L - 3 : 0][s4] = P[1][s4]; }
            }
        }
        if (emit) {
            __syncthreads();
            // store role: this wave's channels are {2 w, 2 w + 1}; whole 128 NG-byte runs of one (channel, band) per half wave / wave
            const unsigned zoff = (unsigned)(iz * plane_cells);
            // (tests/test_cl_drop_resources.py compiles this file and holds every instantiation to zero spills)
            // DROP: the uniform offsets and tile addresses below are formed anew in every step -- kept across the loop (8 bands x
            // 2 channels each, next to the extra descriptors and pointers) they do not fit the scalar registers and were spilled
            int dvs = dvol, ws = w;
            if (DROP) asm volatile("" : "+s"(dvs), "+s"(ws));
#pragma unroll
            for (int sb = 0; sb < 8; ++sb) {
                const unsigned mo = 4u * ((unsigned)((sb > 0 ? sb - 1 : 0) * dvs) + zoff);   // DROP: (band, z) of the factor
                if (NG == 1) {                                    // both channels in one instruction (lane / 32)
                    float* slot = tile + (2 * ws + (lane >> 5)) * CHS + sb * CELLS + (lane & 31);
                    float v = *slot;
                    const unsigned uo = sb == 0 ? 4u * ((unsigned)((c0 + 2 * ws) * dvs) + zoff)
                                                : 4u * ((unsigned)(((c0 + 2 * ws) * 7 + sb - 1) * dvs) + zoff);
                    if (DROP) v = fold(sb, v, sb == 0 ? so0 : soh, uo, som, mo, slot);
                    if (sb == 0) cl_store<false>(v, rb0, so0, uo);
                    else cl_store<false>(v, rbh, soh, uo);
                } else {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int cb = c0 + 2 * ws + h;
                        if (cb >= a.C) continue;
#pragma unroll
                        for (int part = 0; part < NG / 2; ++part) {                   // 64 cells = 256 contiguous bytes each
                            float* slot = tile + (2 * ws + h) * CHS + sb * CELLS + part * 64 + lane;
                            float v = *slot;
                            const unsigned lo = (f0 + part * 64 + lane < plane_cells) ? so0 + 256u * part : kOutside;
                            const unsigned uo = sb == 0 ? 4u * ((unsigned)(cb * dvs) + zoff) : 4u * ((unsigned)((cb * 7 + sb - 1) * dvs) + zoff);
                            if (DROP) v = fold(sb, v, lo, uo, lo, mo, slot);
                            if (sb == 0) cl_store<false>(v, rb0, lo, uo);
                            else cl_store<false>(v, rbh, lo, uo);
                        }
                    }
                }
            }
            if (DROP && (has & 3 * kDMul)) {
                // the tile now holds band coef per channel: sum the CW channels, one atomic per (band, cell).  Channels
                // beyond C add 0, and that rests on the ARITHMETIC role: it marks their source rows kOutside (`live`), so
                // their band values are 0.  NG == 1 overwrites such a slot with 0 * 0 (coef read through kOutside); NG >= 2
                // skips those channels in the store role and the slot keeps that band value 0.
                // The other buffer is written only after the next step's barrier, as before.
                __syncthreads();
#pragma unroll
                for (int idx = threadIdx.x; idx < 8 * CELLS; idx += 32 * CW) {
                    const int sb = idx / CELLS, f = f0 + idx % CELLS;
                    const unsigned bit = sb == 0 ? 1u : 2u;
                    if (!(has & bit * kDMul) || f >= plane_cells) continue;
                    float t = tile[idx];
#pragma unroll
                    for (int c = 1; c < CW; ++c) t += tile[c * CHS + idx];
                    const long long o = (long long)(sb > 0 ? sb - 1 : 0) * dvs + (long long)zoff + f;
                    if ((has & bit * kL1) && cg == 0) {           // the factor again: asked of both arrays like the synthesis does
                        float ml, mh;
                        cl_load(ml, rm0, sb == 0 ? 4u * (unsigned)o : kOutside, 0u);
                        cl_load(mh, rmh, sb > 0 ? 4u * (unsigned)o : kOutside, 0u);
                        const float m = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, ml) | __builtin_bit_cast(unsigned, mh));
                        t += (sb == 0 ? g1l : g1h) * sign_of(m);
                    }
                    atomicAdd((sb == 0 ? a.d_mul_l : a.d_mul_h) + (long long)cg * a.dmul_gstride + o, t);
                }
            }
            buf ^= 1;
        }
    }
}

// z chunk length: few enough workgroups per slot that no round is mostly idle, long enough that the warm-up plane of a
// chunk (read and contracted, nothing emitted) stays a small share.  num_cus: the CU count the cost is formed with.
int pick_zchunk(long long columns, int nz, int slots_per_cu, int num_cus) {
    if (const char* e = getenv("LFGC_CL_NCHUNKS")) { const int nc = atoi(e); if (nc >= 1 && nc <= nz) return (nz + nc - 1) / nc; }   // diagnostics
    const int slots = slots_per_cu * num_cus;
    long long best_cost = -1;
    int best = nz;
    for (int nchunks = 1; nchunks <= nz; ++nchunks) {
        const int zc = (nz + nchunks - 1) / nchunks;
        const long long groups = columns * ((nz + zc - 1) / zc);
        const long long rounds = (groups + slots - 1) / slots;
        const long long cost = rounds * (zc + 1);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = zc; }
    }
    return best;
}

// Launch shape of both kernels once cw, cells, drop and lds_bytes are chosen: plane tiles x channel groups x z chunks of
// `nz` steps, as 8 XCD queues of ceil(total / 8) workgroups (cl_work_item).  slots_per_cu: resident workgroups per CU.
int fill_cl_launch(long long ptiles, int channel_stride, int nz, int slots_per_cu, int num_cus, lfgc_wavelet_cl_plan_info* p) {
    p->ngroups = channel_stride / p->cw;
    if (ptiles * p->ngroups > 0x0fffffffLL) return LFGC_E_UNSUPPORTED;
    p->ptiles = (int)ptiles;
    p->threads = p->cw * kCells;
    p->zchunk = pick_zchunk(ptiles * p->ngroups, nz, slots_per_cu, num_cus > 0 ? num_cus : lfgc_num_cus());
    p->nchunks = (nz + p->zchunk - 1) / p->zchunk;
    const long long total = (long long)p->ptiles * p->ngroups * p->nchunks;
    const long long blocks = (total + 7) / 8 * 8;
    if (blocks > 0x7fffffffLL || p->lds_bytes > 80 * 1024) return LFGC_E_UNSUPPORTED;
    p->blocks = (int)blocks;
    return LFGC_OK;
}

template <auto Kern, typename A>
int launch_cl(const A& a, const lfgc_wavelet_cl_plan_info& p, hipStream_t stream) {
    return lfgc_launch<Kern>(dim3((unsigned)p.blocks), dim3((unsigned)p.threads), p.lds_bytes, stream, a);
}

// drop-layer operands of the two directions (all NULL / NaN: the plain level)
struct ClDropFwd { const float* mul_l; const float* mul_h; float thr_l, thr_h; };
struct ClDropBwd {
    const float* lll; const float* hf; const float* mul_l; const float* mul_h; float* d_mul_l; float* d_mul_h;
    const float* pg[4];    // penalty_grads (include/lfgc.h)
    int gstride;           // AnalysisClArgs::dmul_gstride
};

// Shape checks of both directions (the pointer checks are the entries' own).
int check_cl_shape(int L, int C, int cs, int d0, int d1, int d2, int t0, int t1, int t2) {
    if (L != 2 && L != 4) return LFGC_E_UNSUPPORTED;   // 6- and 8-tap: channel-first kernels + lfgc_grid_layout_f32
    if (C < 1 || d0 < 1 || d1 < 1 || d2 < 1 || t0 < 1 || t1 < 1 || t2 < 1) return LFGC_E_SHAPE;
    if (t0 > 2 * d0 + L - 2 || t1 > 2 * d1 + L - 2 || t2 > 2 * d2 + L - 2) return LFGC_E_SHAPE;
    if (cs != lfgc_roundup(C, 8)) return LFGC_E_SHAPE;
    // buffer descriptors with kOutside as the out-of-range marker: every array below 2^30 bytes
    if ((long long)t0 * t1 * t2 * cs * 4 >= (1LL << 30) || (long long)d0 * d1 * d2 * 7 * C * 4 >= (1LL << 30)) return LFGC_E_UNSUPPORTED;
    return LFGC_OK;
}

int check_cl(const void* p0, const void* p1, const void* p2, const void* p3, const float* taps, int L, int C, int cs,
             int d0, int d1, int d2, int t0, int t1, int t2) {
    if (!p0 || !p1 || !p2 || !p3) return LFGC_E_NULL;
    if (!taps) return LFGC_E_UNSUPPORTED;              // dense stencil: channel-first kernels + lfgc_grid_layout_f32
    return check_cl_shape(L, C, cs, d0, d1, d2, t0, t1, t2);
}

// THE launch selection of the synthesis: idwt_cl launches what *p says and lfgc_idwt_level_cl_plan reports it.
int idwt_cl_select(int K, bool drop, int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2, int num_cus,
                   lfgc_wavelet_cl_plan_info* p) {
    *p = lfgc_wavelet_cl_plan_info{};
    p->drop = drop;
    p->cells = kCells;
    // 32 channels on a large plane: one workgroup of 16 waves writes whole 128-byte lines (d = 65: 197 vs 203 us); on a
    // small one two 8-wave groups balance better (d = 33: 26.5 vs 28.7 us).  24 channels: three groups of 8.
    const long long ptiles = ((long long)(d1 + K - 1) * (d2 + K - 1) + kCells - 1) / kCells;
    int cw = channel_stride == 32 ? (ptiles >= 96 ? 32 : 16) : channel_stride == 16 ? 16 : 8;
    if (const char* e = getenv("LFGC_CL_CW")) { const int v = atoi(e); if ((v == 8 || v == 16 || v == 32) && channel_stride % v == 0) cw = v; }   // diagnostics
    p->cw = cw;
    p->lds_bytes = 2 * 8 * kCells * (cw + 1) * 4 + (drop ? 2 * 8 * K * K * kCells * 4 : 0);    // DROP: + the factor table
    bool nt = cw == 32 && (long long)t0 * t1 * t2 * channel_stride * 4 > (48LL << 20); // see cl_store
    if (const char* e = getenv("LFGC_CL_NT")) nt = e[0] == '1';                         // diagnostics
    p->nt = nt;
    // workgroups per CU: 96 VGPRs, 4 waves per SIMD.  DROP: 101 to 110 VGPRs (Haar: 40), still 4 waves per SIMD, and the
    // 8 KB factor table leaves the LDS count as it is (75.8 KB x 1, 43 KB x 2, 26.4 KB x 4 of 160 KB)
    return fill_cl_launch(ptiles, channel_stride, d0 + K - 1, cw == 32 ? 1 : cw == 16 ? 2 : 4, num_cus, p);
}

// Launch of the selected synthesis shape; DROP picks the instantiation, everything else was decided by idwt_cl_select.
template <int K, bool DROP>
int idwt_cl_launch(const IdwtClArgs<K>& a, const lfgc_wavelet_cl_plan_info& p, hipStream_t st) {
    const bool nt = p.nt != 0;
    if (p.cw == 32) {
        // 67.6 KB of LDS, above the 64 KB default limit: the first use raises BOTH store-policy builds, so that a first
        // launch of the other one inside a later graph capture makes no attribute call
        int rc = lfgc_raise_lds_limit<idwt_cl_kernel<32, kCells, true, K, DROP>>(p.lds_bytes);
        if (rc == LFGC_OK) rc = lfgc_raise_lds_limit<idwt_cl_kernel<32, kCells, false, K, DROP>>(p.lds_bytes);
        if (rc != LFGC_OK) return rc;
        return nt ? launch_cl<idwt_cl_kernel<32, kCells, true, K, DROP>>(a, p, st) : launch_cl<idwt_cl_kernel<32, kCells, false, K, DROP>>(a, p, st);
    }
    if (p.cw == 16) return nt ? launch_cl<idwt_cl_kernel<16, kCells, true, K, DROP>>(a, p, st) : launch_cl<idwt_cl_kernel<16, kCells, false, K, DROP>>(a, p, st);
    return nt ? launch_cl<idwt_cl_kernel<8, kCells, true, K, DROP>>(a, p, st) : launch_cl<idwt_cl_kernel<8, kCells, false, K, DROP>>(a, p, st);
}

template <int K>
int idwt_cl(const float* lll, const float* hf, const ClDropFwd& dr, const float* taps, float* out_cl, int C, int channel_stride,
            int d0, int d1, int d2, int t0, int t1, int t2, hipStream_t st) {
    IdwtClArgs<K> a = {};
    a.lll = lll; a.hf = hf; a.out = out_cl;
    a.C = C; a.cs = channel_stride; a.d0 = d0; a.d1 = d1; a.d2 = d2; a.t0 = t0; a.t1 = t1; a.t2 = t2;
    a.o0 = (2 * d0 + 2 * K - 2 - t0) / 2; a.o1 = (2 * d1 + 2 * K - 2 - t1) / 2; a.o2 = (2 * d2 + 2 * K - 2 - t2) / 2;
    for (int i = 0; i < 4 * K; ++i) a.taps[i] = taps[i];
    a.mul_l = dr.mul_l; a.mul_h = dr.mul_h; a.thr_l = dr.thr_l; a.thr_h = dr.thr_h;
    lfgc_wavelet_cl_plan_info p;
    const int rc = idwt_cl_select(K, dr.mul_l || dr.mul_h, channel_stride, d0, d1, d2, t0, t1, t2, 0, &p);
    if (rc != LFGC_OK) return rc;
    a.zchunk = p.zchunk; a.ptiles = p.ptiles; a.ngroups = p.ngroups; a.nchunks = p.nchunks;
    return p.drop ? idwt_cl_launch<K, true>(a, p, st) : idwt_cl_launch<K, false>(a, p, st);
}

// THE launch selection of the adjoint: idwt_cl_bwd launches what *p says and lfgc_idwt_level_cl_bwd_plan reports it.
int idwt_cl_bwd_select(int K, bool drop, int channel_stride, int d0, int d1, int d2, int num_cus, lfgc_wavelet_cl_plan_info* p) {
    *p = lfgc_wavelet_cl_plan_info{};
    p->drop = drop;
    const int cw = channel_stride % 16 == 0 ? 16 : 8;
    // cells per workgroup: 64 on a large plane (256-byte runs per (channel, band): one whole line + two shared ones per
    // store instead of two shared ones: 188 -> 176 us at d = 65; 128 cells: no further gain), 32 on a small one (d = 33:
    // 23.6 vs 24.2 us, more workgroups)
    int ng = (long long)d1 * d2 >= 3072 ? 2 : 1;
    if (const char* e = getenv("LFGC_CL_ADJ_NG")) { const int v = atoi(e); if (v == 1 || v == 2) ng = v; }   // diagnostics
    p->cw = cw;
    p->cells = kCells * ng;
    const long long ptiles = ((long long)d1 * d2 + kCells * ng - 1) / (kCells * ng);
    // LDS 33 KB x ng per 16 channels; <= 6 waves per SIMD.  DROP has the same tile; db2 with 32-cell tiles runs at 90
    // instead of 76 VGPRs, i.e. 5 waves per SIMD = 20 per CU: two 8-wave or five 4-wave workgroups (64-cell tiles: 109
    // to 111 VGPRs, 4 waves per SIMD as before; Haar: at most 46)
    int slots = cw == 16 ? (ng == 2 ? 2 : 3) : (ng == 2 ? 4 : 6);
    if (drop && K == 2 && ng == 1) slots = cw == 16 ? 2 : 5;
    p->lds_bytes = 2 * cw * (8 * kCells * ng + 1) * 4;
    return fill_cl_launch(ptiles, channel_stride, d0, slots, num_cus, p);
}

template <int K, bool DROP>
int idwt_cl_bwd_launch(const AnalysisClArgs<K>& a, const lfgc_wavelet_cl_plan_info& p, hipStream_t st) {
    if (p.cells == 2 * kCells) return p.cw == 16 ? launch_cl<analysis_cl_kernel<16, 2, K, DROP>>(a, p, st)      // 65.7 KB of LDS
                                                 : launch_cl<analysis_cl_kernel<8, 2, K, DROP>>(a, p, st);
    return p.cw == 16 ? launch_cl<analysis_cl_kernel<16, 1, K, DROP>>(a, p, st) : launch_cl<analysis_cl_kernel<8, 1, K, DROP>>(a, p, st);
}

template <int K>
int idwt_cl_bwd(const float* d_out_cl, const float* taps, const ClDropBwd& dr, float* d_lll, float* d_hf, int C, int channel_stride,
                int d0, int d1, int d2, int t0, int t1, int t2, hipStream_t st) {
    AnalysisClArgs<K> a = {};
    a.src = d_out_cl; a.band0 = d_lll; a.bandh = d_hf;
    a.C = C; a.cs = channel_stride; a.n0 = t0; a.n1 = t1; a.n2 = t2;
    a.lo0 = (2 * d0 + 2 * K - 2 - t0) / 2; a.lo1 = (2 * d1 + 2 * K - 2 - t1) / 2; a.lo2 = (2 * d2 + 2 * K - 2 - t2) / 2;
    a.d0 = d0; a.d1 = d1; a.d2 = d2;
    for (int i = 0; i < 4 * K; ++i) a.taps[i] = taps[i];
    a.lll = dr.lll; a.hf = dr.hf; a.mul_l = dr.mul_l; a.mul_h = dr.mul_h; a.d_mul_l = dr.d_mul_l; a.d_mul_h = dr.d_mul_h;
    a.g_l2_l = dr.pg[0]; a.g_l2_h = dr.pg[1]; a.g_l1_l = dr.pg[2]; a.g_l1_h = dr.pg[3];
    a.dmul_gstride = dr.gstride;
    lfgc_wavelet_cl_plan_info p;
    const int rc = idwt_cl_bwd_select(K, dr.mul_l || dr.mul_h || dr.pg[0] || dr.pg[1], channel_stride, d0, d1, d2, 0, &p);
    if (rc != LFGC_OK) return rc;
    a.zchunk = p.zchunk; a.ptiles = p.ptiles; a.ngroups = p.ngroups; a.nchunks = p.nchunks;
    return p.drop ? idwt_cl_bwd_launch<K, true>(a, p, st) : idwt_cl_bwd_launch<K, false>(a, p, st);
}

// The two entries behind the C ABI: argument checks, then the one dispatch on the filter length.  wide_ok: the plain pair
// takes C > 32 (include/lfgc.h; tests/test_wavelet_cl_paths_gpu.py runs C = 40 and 48), the drop pair refuses it.
int idwt_cl_entry(bool wide_ok, const float* lll, const float* hf, const float* mul_lll, float thr_lll, const float* mul_hf,
                  float thr_hf, const float* taps, int filter_len, float* out_cl, int C, int channel_stride,
                  int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream) {
    const int rc = check_cl(lll, hf, out_cl, out_cl, taps, filter_len, C, channel_stride, d0, d1, d2, t0, t1, t2);
    if (rc != LFGC_OK) return rc;
    if (C > 32 && !wide_ok) return LFGC_E_UNSUPPORTED;             // channel-first DROP level + lfgc_grid_layout_f32
    const ClDropFwd dr = {mul_lll, mul_hf, thr_lll, thr_hf};
    return filter_len == 2 ? idwt_cl<1>(lll, hf, dr, taps, out_cl, C, channel_stride, d0, d1, d2, t0, t1, t2, (hipStream_t)stream)
                           : idwt_cl<2>(lll, hf, dr, taps, out_cl, C, channel_stride, d0, d1, d2, t0, t1, t2, (hipStream_t)stream);
}

int idwt_cl_bwd_entry(bool wide_ok, const float* d_out_cl, const float* taps, int filter_len, const float* lll, const float* hf,
                      const float* mul_lll, const float* mul_hf, float* d_lll, float* d_hf, float* d_mul_lll, float* d_mul_hf,
                      int64_t slice_stride, const float* const* penalty_grads, int C, int channel_stride, int d0, int d1, int d2,
                      int t0, int t1, int t2, lfgc_stream_t stream) {
    ClDropBwd dr = {lll, hf, mul_lll, mul_hf, d_mul_lll, d_mul_hf, {nullptr, nullptr, nullptr, nullptr}, (int)slice_stride};
    if (penalty_grads) for (int i = 0; i < 4; ++i) dr.pg[i] = penalty_grads[i];
    if (!d_out_cl || !d_lll || !d_hf) return LFGC_E_NULL;
    if ((d_mul_lll && (!mul_lll || !lll)) || (d_mul_hf && (!mul_hf || !hf))) return LFGC_E_NULL;
    if ((dr.pg[0] && !lll) || (dr.pg[1] && !hf) || (dr.pg[2] && !d_mul_lll) || (dr.pg[3] && !d_mul_hf)) return LFGC_E_NULL;
    const int rc = check_cl(d_out_cl, d_lll, d_hf, d_hf, taps, filter_len, C, channel_stride, d0, d1, d2, t0, t1, t2);
    if (rc != LFGC_OK) return rc;
    if (C > 32 && !wide_ok) return LFGC_E_UNSUPPORTED;
    // slices of one factor each at least (the detail factor is the larger one); 4 of them stay below 2^30 floats
    if (slice_stride < 0 || slice_stride >= (1LL << 28) ||
        (slice_stride > 0 && slice_stride < (d_mul_hf ? 7 : 1) * (int64_t)d0 * d1 * d2)) return LFGC_E_SHAPE;
    return filter_len == 2 ? idwt_cl_bwd<1>(d_out_cl, taps, dr, d_lll, d_hf, C, channel_stride, d0, d1, d2, t0, t1, t2, (hipStream_t)stream)
                           : idwt_cl_bwd<2>(d_out_cl, taps, dr, d_lll, d_hf, C, channel_stride, d0, d1, d2, t0, t1, t2, (hipStream_t)stream);
}

}  // namespace

extern "C" int lfgc_idwt_level_cl_drop_len_f32(const float* lll, const float* hf, const float* mul_lll, float thr_lll,
                                               const float* mul_hf, float thr_hf, const float* taps, int filter_len,
                                               float* out_cl, int C, int channel_stride, int d0, int d1, int d2,
                                               int t0, int t1, int t2, lfgc_stream_t stream) {
    return idwt_cl_entry(false, lll, hf, mul_lll, thr_lll, mul_hf, thr_hf, taps, filter_len, out_cl, C, channel_stride,
                         d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_cl_drop_bwd_det_len_f32(const float* d_out_cl, const float* taps, int filter_len,
                                                       const float* lll, const float* hf, const float* mul_lll, const float* mul_hf,
                                                       float* d_lll, float* d_hf, float* d_mul_lll, float* d_mul_hf,
                                                       int64_t slice_stride, const float* const* penalty_grads, int C,
                                                       int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2,
                                                       lfgc_stream_t stream) {
    return idwt_cl_bwd_entry(false, d_out_cl, taps, filter_len, lll, hf, mul_lll, mul_hf, d_lll, d_hf, d_mul_lll, d_mul_hf,
                             slice_stride, penalty_grads, C, channel_stride, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_cl_drop_bwd_len_f32(const float* d_out_cl, const float* taps, int filter_len,
                                                   const float* lll, const float* hf, const float* mul_lll, const float* mul_hf,
                                                   float* d_lll, float* d_hf, float* d_mul_lll, float* d_mul_hf,
                                                   const float* const* penalty_grads, int C, int channel_stride,
                                                   int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream) {
    return lfgc_idwt_level_cl_drop_bwd_det_len_f32(d_out_cl, taps, filter_len, lll, hf, mul_lll, mul_hf, d_lll, d_hf, d_mul_lll,
                                                   d_mul_hf, 0, penalty_grads, C, channel_stride, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_cl_len_f32(const float* lll, const float* hf, const float* taps, int filter_len, float* out_cl,
                                          int C, int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2,
                                          lfgc_stream_t stream) {
    return idwt_cl_entry(true, lll, hf, nullptr, 0.0f, nullptr, 0.0f, taps, filter_len, out_cl, C, channel_stride,
                         d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_cl_f32(const float* lll, const float* hf, const float* taps, float* out_cl,
                                      int C, int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2,
                                      lfgc_stream_t stream) {
    return lfgc_idwt_level_cl_len_f32(lll, hf, taps, 4, out_cl, C, channel_stride, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_cl_bwd_len_f32(const float* d_out_cl, const float* taps, int filter_len, float* d_lll, float* d_hf,
                                              int C, int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2,
                                              lfgc_stream_t stream) {
    return idwt_cl_bwd_entry(true, d_out_cl, taps, filter_len, nullptr, nullptr, nullptr, nullptr, d_lll, d_hf, nullptr, nullptr,
                             0, nullptr, C, channel_stride, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_cl_bwd_f32(const float* d_out_cl, const float* taps, float* d_lll, float* d_hf,
                                          int C, int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2,
                                          lfgc_stream_t stream) {
    return lfgc_idwt_level_cl_bwd_len_f32(d_out_cl, taps, 4, d_lll, d_hf, C, channel_stride, d0, d1, d2, t0, t1, t2, stream);
}

// ---- read-only plan queries (include/lfgc.h): the selections above, nothing launched --------------------------------

extern "C" int lfgc_idwt_level_cl_plan(int filter_len, int has_drop, int C, int channel_stride, int d0, int d1, int d2,
                                       int t0, int t1, int t2, int num_cus, lfgc_wavelet_cl_plan_info* out) {
    if (!out) return LFGC_E_NULL;
    const int rc = check_cl_shape(filter_len, C, channel_stride, d0, d1, d2, t0, t1, t2);
    if (rc != LFGC_OK) return rc;
    if (C > 32 && has_drop) return LFGC_E_UNSUPPORTED;
    lfgc_wavelet_cl_plan_info p;
    const int rs = idwt_cl_select(filter_len / 2, has_drop != 0, channel_stride, d0, d1, d2, t0, t1, t2, num_cus, &p);
    if (rs == LFGC_OK) *out = p;
    return rs;
}

extern "C" int lfgc_idwt_level_cl_bwd_plan(int filter_len, int has_drop, int C, int channel_stride, int d0, int d1, int d2,
                                           int t0, int t1, int t2, int num_cus, lfgc_wavelet_cl_plan_info* out) {
    if (!out) return LFGC_E_NULL;
    const int rc = check_cl_shape(filter_len, C, channel_stride, d0, d1, d2, t0, t1, t2);
    if (rc != LFGC_OK) return rc;
    if (C > 32 && has_drop) return LFGC_E_UNSUPPORTED;
    lfgc_wavelet_cl_plan_info p;
    const int rs = idwt_cl_bwd_select(filter_len / 2, has_drop != 0, channel_stride, d0, d1, d2, num_cus, &p);
    if (rs == LFGC_OK) *out = p;
    return rs;
}
