// lfgc_wavelet.hip -- separable-bank 3-D wavelet kernels for gfx950, filter length L = 2K in {2, 4, 6, 8}.
//   lfgc_idwt_level_f32           replaces wavelet_transform/Torch_Wavelet_Transform.py:91-104 (+ crop :69-73)
//   lfgc_idwt_level_bwd_f32       its adjoint (autograd of the same lines)
//   lfgc_idwt_level_drop_f32/_bwd the same two with the pruning layers' per-coefficient factors folded in
//   lfgc_dwt_level_f32            replaces :59-67, :75-89 (init-time encode)
//   (each with a *_len_f32 twin that takes the filter length; the plain names are the 4-tap (db2) entries)
//   lfgc_grid_layout_f32          channel-first <-> channel-last conversion of the dense grid (the sampler and the
//                                 gradient scatter work channel-last, the stencils channel-first)
// All of them are byte movers with a (2K)^3-tap stencil per output (no contraction worth an MFMA).  Both stencils share
// one shape: a workgroup owns 2 z-slices of a run of consecutive cells of the flattened (y,x) plane of ONE channel, copies
// the input neighbourhood of those cells into LDS as plain contiguous chunks of the source rows (every source value
// is fetched from memory once per workgroup instead of once per reading thread: the per-thread version was bound by
// the 64 vector-load instructions each thread issued), then every thread forms its 8 results from LDS with filter
// taps that are broadcast LDS reads.  Boundary handling is a select on the LDS value, never a branch.
// The kernels are templates on the half-length K; the K = 2 instances are the original db2 kernels instruction for
// instruction.  Other lengths take the separable (`taps`) form only: the reference only ever builds outer products.
#include "lfgc_common.h"
#include "lfgc_drop_value.h"   // drop_value(), sign_of()
#include <type_traits>

#ifndef LFGC_WAVELET_ABLATE
#define LFGC_WAVELET_ABLATE 0          // diagnostics (tools/ablate_wavelet.py): 1 no output stores, 2 no arithmetic, 4 no staging loads
#endif

namespace {

template <int K>
struct IdwtArgs {
    const float* lll;   // (C, d0,d1,d2)
    const float* hf;    // (C, 7, d0,d1,d2)
    const float* filt;  // (8,4,4,4) (K = 2 dense build only)
    float* out;         // (C, t0,t1,t2)
    int C, d0, d1, d2, t0, t1, t2, o0, o1, o2;   // o = crop offset floor((2d+2K-2-t)/2)
    int len;            // plane offsets per staged z-plane
    int zchunk;         // sliding-window kernel: output z-slices per workgroup
    float taps[4 * K];  // SEP build: the 1-D bank the filter is the outer product of: [low | high][tap]
    // DROP build only: the pruning layers' per-coefficient factors, shared by all channels
    const float* mul_l; // (d0,d1,d2) or NULL
    const float* mul_h; // (7, d0,d1,d2) or NULL
    float thr_l, thr_h; // NaN: value = x * m;  else masked straight-through: value = (x*(m>=thr) - x*m) + x*m
};

constexpr int kTileCells = 128;      // analysis: cells of the flattened (y,x) plane per z-slice of a workgroup
constexpr int kFwdCells = 256;       // synthesis: plane cells per workgroup (one per thread, both z-slices each)

// Synthesis: out_full[o] = sum_{s,t} in[s][i] F_s[t], o = 2 i + t per axis.  Thread = cell jj in [0,d+K-2] per axis:
// it produces the 2x2x2 outputs o = 2 jj + p from the cells i = jj - e (e in [0,K)) with taps t = p + 2 e.  Haar
// (K = 1) has no neighbour cells: each 2x2x2 output block is an 8-to-8 butterfly of one cell's bands.
// LDS: [512 filter taps as [tap][band] (K = 2 only)] [K+1 z-planes (jz0 - K + 1 + zl)][len plane offsets][12 floats:
// the 8 bands of that cell + pad]; element k is plane offset chunk0 + k, chunk0 = (first cell row - K + 1) * d2 - K + 1.
// The 48-byte records make both the two ds_write_b128 of the staging and the two ds_read_b128 per neighbour cell
// conflict-free (stride 4 * 3 dwords).  Offsets outside the plane (and z-planes outside the level) are staged as zeros,
// so only the x range of a neighbour needs a select.
constexpr int kRec = 12;

constexpr int filt_floats(int K) { return K == 2 ? 512 : 0; }   // the dense 4-tap filter's LDS slot

// x range of neighbour ex of the cell in column jx (cx = jx - ex in [0, d2)); written so that the bounds that always hold
// (jx >= 0, jx - (K-1) < d2) are not tested
template <int K>
__device__ __forceinline__ bool x_in_level(int jx, int ex, int d2) {
    return (ex == 0 || jx >= ex) && (ex == K - 1 || jx - ex < d2);
}

template <bool DROP, bool SEP, int K>
__global__ __launch_bounds__(256) void idwt_level_kernel(const IdwtArgs<K> a) {
    static_assert(SEP || K == 2, "dense (non-separable) filters are 4-tap only");
    constexpr int L = 2 * K;
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    float* s_f = s_dyn;
    float* s_v = s_dyn + filt_floats(K);
    if (!SEP)
        for (int i = threadIdx.x; i < 512; i += 256) s_f[(i & 63) * 8 + (i >> 6)] = a.filt[i];
    const int n0 = a.d0 + (K - 1), n1 = a.d1 + (K - 1), n2 = a.d2 + (K - 1);
    const int plane_cells = n1 * n2;
    const int pt = blockIdx.x, zt = blockIdx.y, c = blockIdx.z;     // 3-D grid: no index divisions
    const int f0 = pt * kFwdCells, jz0 = zt * 2;
    const int chunk0 = (f0 / n2 - (K - 1)) * a.d2 - (K - 1);
    const int len = a.len;
    const int dplane = a.d1 * a.d2;
    const int dvol = dplane * a.d0;                       // < 2^31 / 8 (checked on the host)
    const float* lc = a.lll + (long long)c * dvol;
    const float* hc = a.hf + (long long)c * 7 * dvol;
#pragma unroll 1
    for (int kk = threadIdx.x; kk < len; kk += 256) {
        const int off = chunk0 + kk;
        const bool in_plane = off >= 0 && off < dplane;
        float r[K + 1][8];
#pragma unroll
        for (int zl = 0; zl < K + 1; ++zl) {
            const int iz = jz0 - (K - 1) + zl;
            const bool ok = in_plane && iz >= 0 && iz < a.d0;
            const int o = ok ? iz * dplane + off : 0;
            r[zl][0] = (LFGC_WAVELET_ABLATE & 4) ? (float)o : lc[o];
#pragma unroll
            for (int sb = 1; sb < 8; ++sb) r[zl][sb] = (LFGC_WAVELET_ABLATE & 4) ? (float)(o + sb) : hc[(sb - 1) * dvol + o];
            if (DROP) {
                if (a.mul_l) r[zl][0] = drop_value(r[zl][0], a.mul_l[o], a.thr_l, a.thr_l == a.thr_l);
                if (a.mul_h) {
#pragma unroll
                    for (int sb = 1; sb < 8; ++sb)
                        r[zl][sb] = drop_value(r[zl][sb], a.mul_h[(sb - 1) * dvol + o], a.thr_h, a.thr_h == a.thr_h);
                }
            }
#pragma unroll
            for (int sb = 0; sb < 8; ++sb) r[zl][sb] = ok ? r[zl][sb] : 0.0f;
        }
#pragma unroll
        for (int zl = 0; zl < K + 1; ++zl) {
            float* rec = s_v + (zl * len + kk) * kRec;
            *reinterpret_cast<f32x4*>(rec) = f32x4{r[zl][0], r[zl][1], r[zl][2], r[zl][3]};
            *reinterpret_cast<f32x4*>(rec + 4) = f32x4{r[zl][4], r[zl][5], r[zl][6], r[zl][7]};
        }
    }
    __syncthreads();
    // thread = one cell of the (y,x) plane, for BOTH z-slices of the workgroup: the index arithmetic, the x-range
    // selects' predicates and the shared z-planes' neighbour records are shared by its two output cells
    const int f = f0 + threadIdx.x;
    const bool in_plane = f < plane_cells;
    const int fc = min(f, plane_cells - 1);
    const int jy = fc / n2, jx = fc - jy * n2;
    const int k00 = jy * a.d2 + jx - chunk0;
    bool xok[K];
#pragma unroll
    for (int ex = 0; ex < K; ++ex) xok[ex] = x_in_level<K>(jx, ex, a.d2);
    auto load_plane = [&](int zl, float (&P)[K * K][8]) {   // P[q = ey*K+ex][band] of z-plane zl
#pragma unroll
        for (int q = 0; q < K * K; ++q) {
            const bool ok = xok[q % K];
            const float* rec = s_v + (zl * len + k00 - (q / K) * a.d2 - (q % K)) * kRec;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(rec);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(rec + 4);
            P[q][0] = ok ? lo.x : 0.0f; P[q][1] = ok ? lo.y : 0.0f; P[q][2] = ok ? lo.z : 0.0f; P[q][3] = ok ? lo.w : 0.0f;
            P[q][4] = ok ? hi.x : 0.0f; P[q][5] = ok ? hi.y : 0.0f; P[q][6] = ok ? hi.z : 0.0f; P[q][7] = ok ? hi.w : 0.0f;
        }
    };
    float* outc = a.out + (long long)c * a.t0 * a.t1 * a.t2;
    // K register sets of neighbour records, set zl % K holding z-plane zl
    float S[K][K * K][8];
    // one output cell jz = jz0 + h from its neighbour planes: plane iz = jz - ez is staged plane zl = K - 1 + h - ez
    auto cell = [&](int h) {
        const int jz = jz0 + h;
        const bool valid = in_plane && jz < n0;
        auto V = [&](int ez, int ey, int ex, int sb) -> float { return S[(K - 1 + h - ez) % K][ey * K + ex][sb]; };
        auto store = [&](int p, float val) {
            const int oz = 2 * jz + (p >> 2) - a.o0, oy = 2 * jy + ((p >> 1) & 1) - a.o1, ox = 2 * jx + (p & 1) - a.o2;
            if (valid && oz >= 0 && oz < a.t0 && oy >= 0 && oy < a.t1 && ox >= 0 && ox < a.t2) {
                if (!(LFGC_WAVELET_ABLATE & 1) || val == 1.2345e-30f) outc[(oz * a.t1 + oy) * a.t2 + ox] = val;
            }
        };
        if (LFGC_WAVELET_ABLATE & 2) {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                float t = 0.0f;
#pragma unroll
                for (int s8 = 0; s8 < 8; ++s8) t += V((p >> 2) % K, ((p >> 1) & 1) % K, (p & 1) % K, s8);
                store(p, t);
            }
        } else if constexpr (SEP) {
            // F_s[tz][ty][tx] = T[sz][tz] T[sy][ty] T[sx][tx]: contract x, then y, then z in registers (K = 2: 224 FMAs
            // instead of 512, no filter traffic).  Tap of output parity p and neighbour e along one axis: t = p + 2 e.
            float X[K][K][2][2][2];                           // [ez][ey][sz][sy][px]
#pragma unroll
            for (int q = 0; q < 4 * K * K; ++q) {
                const int ez = q / (4 * K), ey = (q / 4) % K, sz = (q >> 1) & 1, sy = q & 1;
#pragma unroll
                for (int px = 0; px < 2; ++px) {
                    float t = 0.0f;
#pragma unroll
                    for (int ex = 0; ex < K; ++ex)
#pragma unroll
                        for (int sx = 0; sx < 2; ++sx)
                            t = __builtin_fmaf(V(ez, ey, ex, sz * 4 + sy * 2 + sx), a.taps[sx * L + px + 2 * ex], t);
                    X[ez][ey][sz][sy][px] = t;
                }
            }
            float Y[K][2][2][2];                              // [ez][sz][py][px]
#pragma unroll
            for (int q = 0; q < 8 * K; ++q) {
                const int ez = q / 8, sz = (q >> 2) & 1, py = (q >> 1) & 1, px = q & 1;
                float t = 0.0f;
#pragma unroll
                for (int ey = 0; ey < K; ++ey)
#pragma unroll
                    for (int sy = 0; sy < 2; ++sy)
                        t = __builtin_fmaf(X[ez][ey][sz][sy][px], a.taps[sy * L + py + 2 * ey], t);
                Y[ez][sz][py][px] = t;
            }
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int pz = p >> 2, py = (p >> 1) & 1, px = p & 1;
                float t = 0.0f;
#pragma unroll
                for (int ez = 0; ez < K; ++ez)
#pragma unroll
                    for (int sz = 0; sz < 2; ++sz)
                        t = __builtin_fmaf(Y[ez][sz][py][px], a.taps[sz * L + pz + 2 * ez], t);
                store(p, t);
            }
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int pz = p >> 2, py = (p >> 1) & 1, px = p & 1;
                float acc = 0.0f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int ez = e >> 2, ey = (e >> 1) & 1, ex = e & 1;
                    const int tap = ((pz + 2 * ez) * 4 + (py + 2 * ey)) * 4 + (px + 2 * ex);
                    const f32x4 f0v = *reinterpret_cast<const f32x4*>(s_f + tap * 8);
                    const f32x4 f1v = *reinterpret_cast<const f32x4*>(s_f + tap * 8 + 4);
                    acc = __builtin_fmaf(V(ez, ey, ex, 0), f0v.x, acc); acc = __builtin_fmaf(V(ez, ey, ex, 1), f0v.y, acc);
                    acc = __builtin_fmaf(V(ez, ey, ex, 2), f0v.z, acc); acc = __builtin_fmaf(V(ez, ey, ex, 3), f0v.w, acc);
                    acc = __builtin_fmaf(V(ez, ey, ex, 4), f1v.x, acc); acc = __builtin_fmaf(V(ez, ey, ex, 5), f1v.y, acc);
                    acc = __builtin_fmaf(V(ez, ey, ex, 6), f1v.z, acc); acc = __builtin_fmaf(V(ez, ey, ex, 7), f1v.w, acc);
                }
                store(p, acc);      // stored per parity: keeps the filter reads of later parities from being hoisted
            }
        }
    };
#pragma unroll
    for (int zl = K - 1; zl >= 0; --zl) load_plane(zl, S[zl % K]);
    cell(0);                        // outputs of cell jz0: staged planes K-1 .. 0
    load_plane(K, S[K % K]);
    cell(1);                        // cell jz0 + 1: staged planes K .. 1
}

// Synthesis with a SLIDING WINDOW along z (separable filters): a workgroup keeps its 256 plane cells and walks `zchunk`
// output slices; output slice jz needs the coefficient planes jz and jz - 1 only, so each step stages ONE new plane (the
// tiled kernel above stages 3 planes per 2 slices), into a 2-slot LDS ring with one barrier per step, and the loads of
// plane jz + 1 are issued right after the barrier so that they fly under the arithmetic of slice jz.  A thread keeps the
// 4 neighbour records of plane jz in registers: they are the ez = 1 operands of the next step.
// Written for K = 2 (db2): a Haar level stages every plane once in the tiled kernel already, and the register carry of
// the K - 1 previous planes does not fit for K >= 3.
template <bool DROP, int KI>
__global__ __launch_bounds__(256) void idwt_slide_kernel(const IdwtArgs<2> a) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    float* s_v = s_dyn;                                   // ring[2][len][kRec]: a plane is read from LDS only in its own step
    const int n0 = a.d0 + 1, n1 = a.d1 + 1, n2 = a.d2 + 1;
    const int plane_cells = n1 * n2;
    const int pt = blockIdx.x, c = blockIdx.z;
    const int jz_begin = blockIdx.y * a.zchunk, jz_end = min(jz_begin + a.zchunk, n0);
    const int f0 = pt * kFwdCells;
    const int chunk0 = (f0 / n2 - 1) * a.d2 - 1;
    const int len = a.len;
    const int dplane = a.d1 * a.d2;
    const int dvol = dplane * a.d0;
    const float* lc = a.lll + (long long)c * dvol;
    const float* hc = a.hf + (long long)c * 7 * dvol;

    auto load_plane = [&](int iz, float (&r)[KI][8]) {    // plane iz of the 8 bands -> registers (zeros outside the level)
#pragma unroll
        for (int i = 0; i < KI; ++i) {
            const int kk = threadIdx.x + 256 * i;
            const int off = chunk0 + kk;
            const bool ok = kk < len && off >= 0 && off < dplane && iz >= 0 && iz < a.d0;
            const int o = ok ? iz * dplane + off : 0;
            r[i][0] = lc[o];
#pragma unroll
            for (int sb = 1; sb < 8; ++sb) r[i][sb] = hc[(sb - 1) * dvol + o];
            if (DROP) {
                if (a.mul_l) r[i][0] = drop_value(r[i][0], a.mul_l[o], a.thr_l, a.thr_l == a.thr_l);
                if (a.mul_h) {
#pragma unroll
                    for (int sb = 1; sb < 8; ++sb)
                        r[i][sb] = drop_value(r[i][sb], a.mul_h[(sb - 1) * dvol + o], a.thr_h, a.thr_h == a.thr_h);
                }
            }
#pragma unroll
            for (int sb = 0; sb < 8; ++sb) r[i][sb] = ok ? r[i][sb] : 0.0f;
        }
    };
    auto write_plane = [&](int slot, const float (&r)[KI][8]) {
#pragma unroll
        for (int i = 0; i < KI; ++i) {
            const int kk = threadIdx.x + 256 * i;
            if (kk < len) {
                float* rec = s_v + (slot * len + kk) * kRec;
                *reinterpret_cast<f32x4*>(rec) = f32x4{r[i][0], r[i][1], r[i][2], r[i][3]};
                *reinterpret_cast<f32x4*>(rec + 4) = f32x4{r[i][4], r[i][5], r[i][6], r[i][7]};
            }
        }
    };

    const int f = f0 + threadIdx.x;
    const bool in_plane = f < plane_cells;
    const int fc = min(f, plane_cells - 1);
    const int jy = fc / n2, jx = fc - jy * n2;
    const int k00 = jy * a.d2 + jx - chunk0;
    const bool xok0 = jx < a.d2, xok1 = jx >= 1;
    auto read_records = [&](int slot, float (&P)[4][8]) {  // P[q = ey*2+ex][band]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool xok = (q & 1) ? xok1 : xok0;
            const float* rec = s_v + (slot * len + k00 - (q >> 1) * a.d2 - (q & 1)) * kRec;
            const f32x4 lo = *reinterpret_cast<const f32x4*>(rec);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(rec + 4);
            P[q][0] = xok ? lo.x : 0.0f; P[q][1] = xok ? lo.y : 0.0f; P[q][2] = xok ? lo.z : 0.0f; P[q][3] = xok ? lo.w : 0.0f;
            P[q][4] = xok ? hi.x : 0.0f; P[q][5] = xok ? hi.y : 0.0f; P[q][6] = xok ? hi.z : 0.0f; P[q][7] = xok ? hi.w : 0.0f;
        }
    };
    float* outc = a.out + (long long)c * a.t0 * a.t1 * a.t2;
    auto cell = [&](int jz, const float (&E0)[4][8], const float (&E1)[4][8]) {     // E0: plane jz, E1: plane jz - 1
        auto V = [&](int e, int sb) -> float { return (e >> 2) ? E1[e & 3][sb] : E0[e & 3][sb]; };
        float X[2][2][2][2][2];                               // [ez][ey][sz][sy][px]
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int ez = q >> 3, ey = (q >> 2) & 1, sz = (q >> 1) & 1, sy = q & 1;
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                float t = 0.0f;
#pragma unroll
                for (int ex = 0; ex < 2; ++ex)
#pragma unroll
                    for (int sx = 0; sx < 2; ++sx)
                        t = __builtin_fmaf(V(ez * 4 + ey * 2 + ex, sz * 4 + sy * 2 + sx), a.taps[sx * 4 + px + 2 * ex], t);
                X[ez][ey][sz][sy][px] = t;
            }
        }
        float Y[2][2][2][2];                                  // [ez][sz][py][px]
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int ez = q >> 3, sz = (q >> 2) & 1, py = (q >> 1) & 1, px = q & 1;
            float t = 0.0f;
#pragma unroll
            for (int ey = 0; ey < 2; ++ey)
#pragma unroll
                for (int sy = 0; sy < 2; ++sy)
                    t = __builtin_fmaf(X[ez][ey][sz][sy][px], a.taps[sy * 4 + py + 2 * ey], t);
            Y[ez][sz][py][px] = t;
        }
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int pz = p >> 2, py = (p >> 1) & 1, px = p & 1;
            float t = 0.0f;
#pragma unroll
            for (int ez = 0; ez < 2; ++ez)
#pragma unroll
                for (int sz = 0; sz < 2; ++sz)
                    t = __builtin_fmaf(Y[ez][sz][py][px], a.taps[sz * 4 + pz + 2 * ez], t);
            const int oz = 2 * jz + pz - a.o0, oy = 2 * jy + py - a.o1, ox = 2 * jx + px - a.o2;
            if (in_plane && oz >= 0 && oz < a.t0 && oy >= 0 && oy < a.t1 && ox >= 0 && ox < a.t2)
                outc[(oz * a.t1 + oy) * a.t2 + ox] = t;
        }
    };

    float r[KI][8];
    float PA[4][8], PB[4][8];
    load_plane(jz_begin - 1, r);
    write_plane((jz_begin + 1) & 1, r);                   // slot of plane jz_begin - 1
    load_plane(jz_begin, r);
    __syncthreads();
    read_records((jz_begin + 1) & 1, PB);                 // plane jz_begin - 1: the first step's ez = 1 operands
    // two steps per trip so that the register sets alternate roles without copies
#pragma unroll 1
    for (int jz = jz_begin; jz < jz_end; jz += 2) {
        write_plane(jz & 1, r);
        __syncthreads();
        if (jz + 1 < jz_end) load_plane(jz + 1, r);       // in flight under this slice's arithmetic
        read_records(jz & 1, PA);
        cell(jz, PA, PB);
        if (jz + 1 < jz_end) {
            write_plane((jz + 1) & 1, r);
            __syncthreads();
            if (jz + 2 < jz_end) load_plane(jz + 2, r);
            read_records((jz + 1) & 1, PB);
            cell(jz + 1, PB, PA);
        }
    }
}

// Analysis-form kernel shared by the IDWT adjoint and the forward DWT:
//   band_s[c][i] = sum_t src_full[c][2 i + t] * F_s[t],  src_full[u] = src[u - lo] (0 outside [0, n))
// DROP (adjoint with the pruning factors):  stored gradient = band_s * m_s,  d_m_s[i] += band_s[c][i] * coef_s[c][i]
// (float atomics over the channels: whole 256-byte rows per wave instruction, 8..32 adds per address).
// LDS: [512 taps (K = 2 only)] [2K+2 chunks (source z-plane 2 iz0 - lo0 + zl) of `len` floats]; chunk element k is
// plane offset chunk0 + k, chunk0 = (2 * first cell row - lo1) * n2 - lo2.
template <int K>
struct AnalysisArgs {
    const float* src;      // (C, n0,n1,n2)
    const float* filt;
    float* band0;          // band 0 of channel c at band0 + c * cstride0
    float* bandh;          // band s>=1 of channel c at bandh + c * cstrideh + (s-1) * dvol
    long long cstride0, cstrideh;
    int C, n0, n1, n2, lo0, lo1, lo2, d0, d1, d2;
    int len;
    float taps[4 * K];     // SEP build: [low | high][tap]
    // DROP build only
    const float* lll;      // forward inputs (C, d0,d1,d2), (C, 7, d0,d1,d2): needed for d_mul
    const float* hf;
    const float* mul_l;    // (d0,d1,d2) or NULL
    const float* mul_h;    // (7, d0,d1,d2) or NULL
    float* d_mul_l;        // (d0,d1,d2) or NULL, pre-zeroed
    float* d_mul_h;        // (7, d0,d1,d2) or NULL, pre-zeroed
    long long dmul_cstride;   // 0: every channel adds into the one d_mul_l / d_mul_h array (float atomics over the channels);
                              // else channel c adds into its own slice d_mul_* + c * dmul_cstride: one add onto zero per
                              // address, exact in any order (lfgc_sum_slices_f32 folds the slices in channel order)
    // penalty gradients folded in (device scalars or NULL): upstream gradient of  sum coef^2  of the low / detail tensor
    // (adds 2 g coef to its gradient) and of  sum |factor|  of a factor that is itself the penalised parameter
    // (Smallify beta: adds g sign(factor) to the factor gradient, once, by the channel-0 workgroups)
    const float* g_l2_l; const float* g_l2_h; const float* g_l1_l; const float* g_l1_h;
};

template <bool DROP, bool SEP, int K>
__global__ __launch_bounds__(256) void analysis_kernel(const AnalysisArgs<K> a) {
    static_assert(SEP || K == 2, "dense (non-separable) filters are 4-tap only");
    constexpr int L = 2 * K;
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    float* s_f = s_dyn;
    float* s_v = s_dyn + filt_floats(K);
    if (!SEP)
        for (int i = threadIdx.x; i < 512; i += 256) s_f[(i & 63) * 8 + (i >> 6)] = a.filt[i];
    const int plane_cells = a.d1 * a.d2;
    const int pt = blockIdx.x, zt = blockIdx.y, c = blockIdx.z;     // 3-D grid: no index divisions
    const int f0 = pt * kTileCells, iz0 = zt * 2;
    const int chunk0 = (2 * (f0 / a.d2) - a.lo1) * a.n2 - a.lo2;
    const int len = a.len;
    const int nplane = a.n1 * a.n2;
    const long long dvol = (long long)plane_cells * a.d0;
    const float* src = a.src + (long long)c * nplane * a.n0;              // per-channel offsets fit 32 bits (host check)
#pragma unroll 2
    for (int kk = threadIdx.x; kk < len; kk += 256) {
        const int off = chunk0 + kk;
        const bool in_plane = off >= 0 && off < nplane;
        float r[L + 2];
#pragma unroll
        for (int zl = 0; zl < L + 2; ++zl) {
            const int uz = 2 * iz0 - a.lo0 + zl;
            const bool ok = in_plane && uz >= 0 && uz < a.n0;
            const float x = src[ok ? uz * nplane + off : 0];
            r[zl] = ok ? x : 0.0f;
        }
#pragma unroll
        for (int zl = 0; zl < L + 2; ++zl) s_v[zl * len + kk] = r[zl];
    }
    __syncthreads();
    const int zl_t = threadIdx.x >> 7;
    const int f = f0 + (threadIdx.x & (kTileCells - 1));
    const int iz = iz0 + zl_t;
    const bool valid = f < plane_cells && iz < a.d0;
    const int fc = min(f, plane_cells - 1);
    const int iy = fc / a.d2, ix = fc - iy * a.d2;
    float acc[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) acc[s] = 0.0f;
    // every tap of a valid cell lies inside the staged chunk; rows / planes outside the source were staged as zeros,
    // so only the x range needs a select
    const int k0 = (2 * iy - a.lo1) * a.n2 + (2 * ix - a.lo2) - chunk0;
    bool xok[L];
#pragma unroll
    for (int tx = 0; tx < L; ++tx) { const int ux = 2 * ix + tx - a.lo2; xok[tx] = ux >= 0 && ux < a.n2; }
    if constexpr (SEP) {
        // contract x, then y, then z (see idwt_level_kernel): band s = 4 sz + 2 sy + sx
        float Y[L][2][2];                                 // [tz][sy][sx]
#pragma unroll
        for (int tz = 0; tz < L; ++tz) {
            const float* pl = s_v + (2 * zl_t + tz) * len + k0;
            float X[L][2];                                // [ty][sx]
#pragma unroll
            for (int ty = 0; ty < L; ++ty) {
                const float* row = pl + ty * a.n2;
                float x0 = 0.0f, x1 = 0.0f;
#pragma unroll
                for (int tx = 0; tx < L; ++tx) {
                    const float raw = row[tx];                  // always in the chunk: load first, then select (a ternary
                    const float val = xok[tx] ? raw : 0.0f;     // around the load compiles to an exec-masked branch per tap)
                    x0 = __builtin_fmaf(val, a.taps[tx], x0);
                    x1 = __builtin_fmaf(val, a.taps[L + tx], x1);
                }
                X[ty][0] = x0; X[ty][1] = x1;
            }
#pragma unroll
            for (int sy = 0; sy < 2; ++sy)
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    float t = 0.0f;
#pragma unroll
                    for (int ty = 0; ty < L; ++ty) t = __builtin_fmaf(X[ty][sx], a.taps[sy * L + ty], t);
                    Y[tz][sy][sx] = t;
                }
        }
#pragma unroll
        for (int sb = 0; sb < 8; ++sb) {
            float t = 0.0f;
#pragma unroll
            for (int tz = 0; tz < L; ++tz) t = __builtin_fmaf(Y[tz][(sb >> 1) & 1][sb & 1], a.taps[(sb >> 2) * L + tz], t);
            acc[sb] = t;
        }
    } else {
#pragma unroll 1                      // a rolled z-tap loop keeps the live filter taps to one 16-tap plane
    for (int tz = 0; tz < 4; ++tz) {
        const float* pl = s_v + (2 * zl_t + tz) * len + k0;
        float v[16];
#pragma unroll
        for (int ty = 0; ty < 4; ++ty) {
            const float* row = pl + ty * a.n2;
#pragma unroll
            for (int tx = 0; tx < 4; ++tx) { const float raw = row[tx]; v[ty * 4 + tx] = xok[tx] ? raw : 0.0f; }
        }
#pragma unroll
        for (int tyx = 0; tyx < 16; ++tyx) {
            const f32x4 f0v = *reinterpret_cast<const f32x4*>(s_f + (tz * 16 + tyx) * 8);
            const f32x4 f1v = *reinterpret_cast<const f32x4*>(s_f + (tz * 16 + tyx) * 8 + 4);
            acc[0] = __builtin_fmaf(v[tyx], f0v.x, acc[0]); acc[1] = __builtin_fmaf(v[tyx], f0v.y, acc[1]);
            acc[2] = __builtin_fmaf(v[tyx], f0v.z, acc[2]); acc[3] = __builtin_fmaf(v[tyx], f0v.w, acc[3]);
            acc[4] = __builtin_fmaf(v[tyx], f1v.x, acc[4]); acc[5] = __builtin_fmaf(v[tyx], f1v.y, acc[5]);
            acc[6] = __builtin_fmaf(v[tyx], f1v.z, acc[6]); acc[7] = __builtin_fmaf(v[tyx], f1v.w, acc[7]);
        }
    }
    }
    if (valid) {
        const long long sp = (long long)iz * plane_cells + fc;
        if (DROP) {
            if (a.mul_l || a.g_l2_l) {
                const float x = (a.d_mul_l || a.g_l2_l) ? a.lll[(long long)c * dvol + sp] : 0.0f;
                if (a.mul_l) {
                    const float m = a.mul_l[sp];
                    if (a.d_mul_l) atomicAdd(a.d_mul_l + c * a.dmul_cstride + sp, acc[0] * x + ((a.g_l1_l && c == 0) ? *a.g_l1_l * sign_of(m) : 0.0f));
                    acc[0] *= m;
                }
                if (a.g_l2_l) acc[0] = __builtin_fmaf(2.0f * *a.g_l2_l, x, acc[0]);
            }
            if (a.mul_h || a.g_l2_h) {
                const float g2 = a.g_l2_h ? 2.0f * *a.g_l2_h : 0.0f;
                const float g1 = (a.g_l1_h && c == 0) ? *a.g_l1_h : 0.0f;
#pragma unroll
                for (int s = 1; s < 8; ++s) {
                    const long long o = (long long)(s - 1) * dvol + sp;
                    const float x = (a.d_mul_h || a.g_l2_h) ? a.hf[(long long)c * 7 * dvol + o] : 0.0f;
                    if (a.mul_h) {
                        const float m = a.mul_h[o];
                        if (a.d_mul_h) atomicAdd(a.d_mul_h + c * a.dmul_cstride + o, acc[s] * x + g1 * sign_of(m));
                        acc[s] *= m;
                    }
                    acc[s] = __builtin_fmaf(g2, x, acc[s]);
                }
            }
        }
        a.band0[(long long)c * a.cstride0 + sp] = acc[0];
#pragma unroll
        for (int s = 1; s < 8; ++s) a.bandh[(long long)c * a.cstrideh + (long long)(s - 1) * dvol + sp] = acc[s];
    }
}

// (C, V) <-> (V, Cs) through a 32(channel) x 64(voxel) LDS tile: both sides move whole 128/256-byte rows.
__global__ __launch_bounds__(256) void first_to_last_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            int C, long long V, int cs) {
    __shared__ float tile[32][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;          // 64 x 4
    const long long v0 = (long long)blockIdx.x * 64;
    for (int c0 = 0; c0 < cs; c0 += 32) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = c0 + ty * 8 + k;
            const long long v = v0 + tx;
            tile[ty * 8 + k][tx] = (c < C && v < V) ? src[(long long)c * V + v] : 0.0f;
        }
        __syncthreads();
        const int cc = threadIdx.x & 31, vv = threadIdx.x >> 5;       // 32 x 8
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long v = v0 + vv * 8 + k;
            if (v < V && c0 + cc < cs) dst[v * cs + c0 + cc] = tile[cc][vv * 8 + k];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void last_to_first_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                            int C, long long V, int cs) {
    __shared__ float tile[32][65];
    const long long v0 = (long long)blockIdx.x * 64;
    for (int c0 = 0; c0 < C; c0 += 32) {
        const int cc = threadIdx.x & 31, vv = threadIdx.x >> 5;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long v = v0 + vv * 8 + k;
            tile[cc][vv * 8 + k] = (v < V && c0 + cc < cs) ? src[v * cs + c0 + cc] : 0.0f;
        }
        __syncthreads();
        const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = c0 + ty * 8 + k;
            const long long v = v0 + tx;
            if (c < C && v < V) dst[(long long)c * V + v] = tile[ty * 8 + k][tx];
        }
        __syncthreads();
    }
}

// filter_len -> K, or 0 for a length without kernels; a dense (non-separable) filter must be 4-tap
inline int half_len(int filter_len, bool has_taps) {
    if (filter_len != 2 && filter_len != 4 && filter_len != 6 && filter_len != 8) return 0;
    if (!has_taps && filter_len != 4) return 0;
    return filter_len / 2;
}

inline int check_level_shape(int L, int C, int d0, int d1, int d2, int t0, int t1, int t2) {
    if (C < 1 || d0 < 1 || d1 < 1 || d2 < 1 || t0 < 1 || t1 < 1 || t2 < 1) return LFGC_E_SHAPE;
    if (t0 > 2 * d0 + L - 2 || t1 > 2 * d1 + L - 2 || t2 > 2 * d2 + L - 2) return LFGC_E_SHAPE;
    return LFGC_OK;
}

inline int check_level(const void* a, const void* b, const void* c, const void* d, int L, int C, int d0, int d1, int d2,
                       int t0, int t1, int t2) {
    if (!a || !b || !c || !d) return LFGC_E_NULL;
    return check_level_shape(L, C, d0, d1, d2, t0, t1, t2);
}

// Runs f(std::bool_constant<drop>): the DROP template argument of the level kernels.
template <typename F>
int with_drop(bool drop, F&& f) {
    return drop ? f(std::true_type()) : f(std::false_type());
}

// Launch shape of every level kernel: `ptiles` plane tiles x `ztiles` z tiles x C channels with `lds` bytes of dynamic LDS
// (all 64-bit here: a long row overflows 32 bits long before it fits).  The staged rows must fit 160 KB.
inline int fill_launch(long long ptiles, long long ztiles, int C, long long len, long long lds, lfgc_wavelet_plan_info* p) {
    if (ptiles > 0x7fffffffLL || ztiles > 65535 || C > 65535 || lds > 160 * 1024) return LFGC_E_UNSUPPORTED;
    p->len = (int)len; p->lds_bytes = (int)lds;
    p->grid[0] = (unsigned)ptiles; p->grid[1] = (unsigned)ztiles; p->grid[2] = (unsigned)C;
    return LFGC_OK;
}

// THE kernel selection of the synthesis: launch_idwt launches what *p says and lfgc_idwt_level_plan reports it.
inline int idwt_select(int K, bool has_taps, bool drop, int C, int d0, int d1, int d2, int t0, int t1, int t2,
                       lfgc_wavelet_plan_info* p) {
    *p = lfgc_wavelet_plan_info{};
    p->drop = drop;
    const int n0 = d0 + K - 1, n1 = d1 + K - 1, n2 = d2 + K - 1;
    const int span = (kFwdCells + n2 - 2) / n2;             // rows a run of 256 cells can straddle beyond its first
    const long long len = (long long)(span + K) * d2 + 2 * K - 2;
    const long long ptiles = ((long long)n1 * n2 + kFwdCells - 1) / kFwdCells;
    if ((long long)d0 * d1 * d2 > 0x7fffffffLL / 8 || (long long)t0 * t1 * t2 > 0x7fffffffLL) return LFGC_E_UNSUPPORTED;
    if (K == 2) {
        const long long ki = (len + 255) / 256;
        // Small levels (<= 40 000 output voxels per channel: everything below the last two levels of a 64^3 grid) take the tiled
        // kernel below: one load -> barrier -> stencil -> store round per workgroup instead of a z walk whose every step waits
        // for a plane (the arithmetic that should hide it is nothing at these sizes): cfg-3 train step 0.385 -> 0.378 ms.
        const bool small_level = (long long)t0 * t1 * t2 <= 40000;
        if (has_taps && ki <= 3 && !small_level) {           // separable filter: sliding window along z
            p->kernel = LFGC_WAVELET_SLIDING_WINDOW;
            p->ki = (int)ki;
            p->zchunk = n0 < 6 ? n0 : 5;
            return fill_launch(ptiles, (n0 + p->zchunk - 1) / p->zchunk, C, len, 2 * len * kRec * 4, p);
        }
    }
    p->kernel = has_taps ? LFGC_WAVELET_TILED_SEPARABLE : LFGC_WAVELET_TILED_DENSE;
    return fill_launch(ptiles, (n0 + 1) / 2, C, len, (filt_floats(K) + (K + 1) * len * kRec) * 4, p);
}

template <int K>
int launch_idwt(IdwtArgs<K> a, bool drop, const float* taps, hipStream_t stream) {
    if (taps) for (int i = 0; i < 4 * K; ++i) a.taps[i] = taps[i];
    a.o0 = (2 * a.d0 + 2 * K - 2 - a.t0) / 2; a.o1 = (2 * a.d1 + 2 * K - 2 - a.t1) / 2; a.o2 = (2 * a.d2 + 2 * K - 2 - a.t2) / 2;
    lfgc_wavelet_plan_info p;
    const int rc = idwt_select(K, taps != nullptr, drop, a.C, a.d0, a.d1, a.d2, a.t0, a.t1, a.t2, &p);
    if (rc != LFGC_OK) return rc;
    a.len = p.len;
    a.zchunk = p.zchunk;
    const dim3 blocks(p.grid[0], p.grid[1], p.grid[2]);
    return with_drop(p.drop, [&](auto dc) {
        constexpr bool DROP = decltype(dc)::value;
        if constexpr (K == 2) {
            if (p.kernel == LFGC_WAVELET_SLIDING_WINDOW) {
                if (p.ki == 1) return lfgc_launch<idwt_slide_kernel<DROP, 1>>(blocks, dim3(256), p.lds_bytes, stream, a);
                if (p.ki == 2) return lfgc_launch<idwt_slide_kernel<DROP, 2>>(blocks, dim3(256), p.lds_bytes, stream, a);
                return lfgc_launch<idwt_slide_kernel<DROP, 3>>(blocks, dim3(256), p.lds_bytes, stream, a);
            }
            if (p.kernel == LFGC_WAVELET_TILED_DENSE)
                return lfgc_launch<idwt_level_kernel<DROP, false, K>>(blocks, dim3(256), p.lds_bytes, stream, a);
        }
        return lfgc_launch<idwt_level_kernel<DROP, true, K>>(blocks, dim3(256), p.lds_bytes, stream, a);
    });
}

// THE kernel selection of the analysis form (adjoint of a level: source extents n = t, lo = the crop offset; forward DWT:
// lo = L - 2): launch_analysis launches what *p says and lfgc_idwt_level_bwd_plan / lfgc_dwt_level_plan report it.
inline int analysis_select(int K, bool has_taps, bool drop, int C, int n0, int n1, int n2, int d0, int d1, int d2,
                           lfgc_wavelet_plan_info* p) {
    *p = lfgc_wavelet_plan_info{};
    p->drop = drop;
    p->kernel = has_taps ? LFGC_WAVELET_ANALYSIS_SEPARABLE : LFGC_WAVELET_ANALYSIS_DENSE;
    const int span = (kTileCells + d2 - 2) / d2;
    const long long len = (long long)(2 * span + 2 * K - 1) * n2 + 2 * d2 + 2 * K - 2;
    const long long ptiles = ((long long)d1 * d2 + kTileCells - 1) / kTileCells;
    if ((long long)n0 * n1 * n2 > 0x7fffffffLL) return LFGC_E_UNSUPPORTED;
    return fill_launch(ptiles, (d0 + 1) / 2, C, len, (filt_floats(K) + (2 * K + 2) * len) * 4, p);
}

template <int K>
int launch_analysis(AnalysisArgs<K> a, bool drop, const float* taps, hipStream_t stream) {
    if (taps) for (int i = 0; i < 4 * K; ++i) a.taps[i] = taps[i];
    lfgc_wavelet_plan_info p;
    const int rc = analysis_select(K, taps != nullptr, drop, a.C, a.n0, a.n1, a.n2, a.d0, a.d1, a.d2, &p);
    if (rc != LFGC_OK) return rc;
    a.len = p.len;
    const dim3 blocks(p.grid[0], p.grid[1], p.grid[2]);
    return with_drop(p.drop, [&](auto dc) {
        constexpr bool DROP = decltype(dc)::value;
        if constexpr (K == 2) {
            if (p.kernel == LFGC_WAVELET_ANALYSIS_DENSE)
                return lfgc_launch<analysis_kernel<DROP, false, K>>(blocks, dim3(256), p.lds_bytes, stream, a);
        }
        return lfgc_launch<analysis_kernel<DROP, true, K>>(blocks, dim3(256), p.lds_bytes, stream, a);
    });
}

// extents of one forward-DWT level: _get_padding_size (Torch_Wavelet_Transform.py:59-63): (2L-3)//2 = L-2 on both sides,
// plus the odd bit on the high side; F.pad slots are (last axis lo, hi, ..., first axis lo, hi) while is_odd is indexed
// first axis first -> the odd bit of axis a pads axis 2-a.
inline void dwt_extents(int filter_len, int n0, int n1, int n2, int* d0, int* d1, int* d2) {
    const int lo = filter_len - 2;
    const int hi0 = lo + (n2 & 1), hi1 = lo + (n1 & 1), hi2 = lo + (n0 & 1);
    *d0 = (n0 + lo + hi0 - filter_len) / 2 + 1; *d1 = (n1 + lo + hi1 - filter_len) / 2 + 1; *d2 = (n2 + lo + hi2 - filter_len) / 2 + 1;
}

// Runs f(std::integral_constant<int, K>) for the half-length K of filter_len (half_len() != 0 checked by the caller).
template <typename F>
int with_half_len(int K, F&& f) {
    switch (K) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
    }
    return LFGC_E_UNSUPPORTED;
}

template <int K>
AnalysisArgs<K> adjoint_args(const float* d_out, const float* filter_rev, float* d_lll, float* d_hf,
                             int C, int d0, int d1, int d2, int t0, int t1, int t2) {
    AnalysisArgs<K> a = {};
    a.src = d_out; a.filt = filter_rev; a.band0 = d_lll; a.bandh = d_hf;
    const long long dvol = (long long)d0 * d1 * d2;
    a.cstride0 = dvol; a.cstrideh = 7 * dvol;
    a.C = C; a.n0 = t0; a.n1 = t1; a.n2 = t2;
    a.lo0 = (2 * d0 + 2 * K - 2 - t0) / 2; a.lo1 = (2 * d1 + 2 * K - 2 - t1) / 2; a.lo2 = (2 * d2 + 2 * K - 2 - t2) / 2;
    a.d0 = d0; a.d1 = d1; a.d2 = d2;
    return a;
}

}  // namespace

extern "C" int lfgc_idwt_level_drop_len_f32(const float* lll, const float* hf, const float* mul_lll, float thr_lll,
                                            const float* mul_hf, float thr_hf, const float* filter_rev, const float* taps,
                                            int filter_len, float* out, int C, int d0, int d1, int d2, int t0, int t1, int t2,
                                            lfgc_stream_t stream) {
    const int K = half_len(filter_len, taps != nullptr);
    if (!K) return LFGC_E_UNSUPPORTED;
    const int rc = check_level(lll, hf, taps ? (const void*)taps : (const void*)filter_rev, out, filter_len, C, d0, d1, d2, t0, t1, t2);
    if (rc != LFGC_OK) return rc;
    return with_half_len(K, [&](auto kc) {
        constexpr int KK = decltype(kc)::value;
        IdwtArgs<KK> a = {};
        a.lll = lll; a.hf = hf; a.filt = filter_rev; a.out = out;
        a.C = C; a.d0 = d0; a.d1 = d1; a.d2 = d2; a.t0 = t0; a.t1 = t1; a.t2 = t2;
        a.mul_l = mul_lll; a.mul_h = mul_hf; a.thr_l = thr_lll; a.thr_h = thr_hf;
        return launch_idwt<KK>(a, mul_lll || mul_hf, taps, (hipStream_t)stream);
    });
}

extern "C" int lfgc_idwt_level_len_f32(const float* lll, const float* hf, const float* filter_rev, const float* taps,
                                       int filter_len, float* out, int C, int d0, int d1, int d2, int t0, int t1, int t2,
                                       lfgc_stream_t stream) {
    return lfgc_idwt_level_drop_len_f32(lll, hf, nullptr, 0.0f, nullptr, 0.0f, filter_rev, taps, filter_len, out,
                                        C, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_f32(const float* lll, const float* hf, const float* filter_rev, const float* taps, float* out,
                                   int C, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream) {
    return lfgc_idwt_level_len_f32(lll, hf, filter_rev, taps, 4, out, C, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_drop_f32(const float* lll, const float* hf, const float* mul_lll, float thr_lll,
                                        const float* mul_hf, float thr_hf, const float* filter_rev, const float* taps, float* out,
                                        int C, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream) {
    return lfgc_idwt_level_drop_len_f32(lll, hf, mul_lll, thr_lll, mul_hf, thr_hf, filter_rev, taps, 4, out,
                                        C, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_drop_bwd_det_len_f32(const float* d_out, const float* filter_rev, const float* taps, int filter_len,
                                                    const float* lll, const float* hf, const float* mul_lll, const float* mul_hf,
                                                    float* d_lll, float* d_hf, float* d_mul_lll, float* d_mul_hf,
                                                    int64_t slice_stride, const float* const* penalty_grads, int C,
                                                    int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream) {
    const int K = half_len(filter_len, taps != nullptr);
    if (!K) return LFGC_E_UNSUPPORTED;
    const int rc = check_level(d_out, taps ? (const void*)taps : (const void*)filter_rev, d_lll, d_hf, filter_len, C, d0, d1, d2, t0, t1, t2);
    if (rc != LFGC_OK) return rc;
    if ((d_mul_lll && (!mul_lll || !lll)) || (d_mul_hf && (!mul_hf || !hf))) return LFGC_E_NULL;
    const float* pg[4] = {nullptr, nullptr, nullptr, nullptr};
    if (penalty_grads) for (int i = 0; i < 4; ++i) pg[i] = penalty_grads[i];
    if ((pg[0] && !lll) || (pg[1] && !hf) || (pg[2] && !d_mul_lll) || (pg[3] && !d_mul_hf)) return LFGC_E_NULL;
    // slices of one factor each at least: the detail factor is the larger one
    if (slice_stride < 0 || (slice_stride > 0 && slice_stride < (d_mul_hf ? 7 : 1) * (int64_t)d0 * d1 * d2)) return LFGC_E_SHAPE;
    return with_half_len(K, [&](auto kc) {
        constexpr int KK = decltype(kc)::value;
        AnalysisArgs<KK> a = adjoint_args<KK>(d_out, filter_rev, d_lll, d_hf, C, d0, d1, d2, t0, t1, t2);
        a.dmul_cstride = slice_stride;
        a.lll = lll; a.hf = hf; a.mul_l = mul_lll; a.mul_h = mul_hf; a.d_mul_l = d_mul_lll; a.d_mul_h = d_mul_hf;
        a.g_l2_l = pg[0]; a.g_l2_h = pg[1]; a.g_l1_l = pg[2]; a.g_l1_h = pg[3];
        return launch_analysis<KK>(a, mul_lll || mul_hf || pg[0] || pg[1], taps, (hipStream_t)stream);
    });
}

extern "C" int lfgc_idwt_level_drop_bwd_len_f32(const float* d_out, const float* filter_rev, const float* taps, int filter_len,
                                                const float* lll, const float* hf, const float* mul_lll, const float* mul_hf,
                                                float* d_lll, float* d_hf, float* d_mul_lll, float* d_mul_hf,
                                                const float* const* penalty_grads, int C, int d0, int d1, int d2,
                                                int t0, int t1, int t2, lfgc_stream_t stream) {
    return lfgc_idwt_level_drop_bwd_det_len_f32(d_out, filter_rev, taps, filter_len, lll, hf, mul_lll, mul_hf, d_lll, d_hf,
                                                d_mul_lll, d_mul_hf, 0, penalty_grads, C, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_bwd_len_f32(const float* d_out, const float* filter_rev, const float* taps, int filter_len,
                                           float* d_lll, float* d_hf, int C, int d0, int d1, int d2, int t0, int t1, int t2,
                                           lfgc_stream_t stream) {
    return lfgc_idwt_level_drop_bwd_len_f32(d_out, filter_rev, taps, filter_len, nullptr, nullptr, nullptr, nullptr, d_lll, d_hf,
                                            nullptr, nullptr, nullptr, C, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_bwd_f32(const float* d_out, const float* filter_rev, const float* taps, float* d_lll, float* d_hf,
                                       int C, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream) {
    return lfgc_idwt_level_bwd_len_f32(d_out, filter_rev, taps, 4, d_lll, d_hf, C, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_idwt_level_drop_bwd_f32(const float* d_out, const float* filter_rev, const float* taps, const float* lll, const float* hf,
                                            const float* mul_lll, const float* mul_hf, float* d_lll, float* d_hf,
                                            float* d_mul_lll, float* d_mul_hf, const float* const* penalty_grads,
                                            int C, int d0, int d1, int d2,
                                            int t0, int t1, int t2, lfgc_stream_t stream) {
    return lfgc_idwt_level_drop_bwd_len_f32(d_out, filter_rev, taps, 4, lll, hf, mul_lll, mul_hf, d_lll, d_hf, d_mul_lll,
                                            d_mul_hf, penalty_grads, C, d0, d1, d2, t0, t1, t2, stream);
}

extern "C" int lfgc_dwt_level_len_f32(const float* in, const float* filter_fwd, const float* taps, int filter_len, float* out,
                                      int C, int n0, int n1, int n2, lfgc_stream_t stream) {
    if (!in || (!filter_fwd && !taps) || !out) return LFGC_E_NULL;
    const int K = half_len(filter_len, taps != nullptr);
    if (!K) return LFGC_E_UNSUPPORTED;
    if (C < 1 || n0 < 1 || n1 < 1 || n2 < 1) return LFGC_E_SHAPE;
    const int lo = filter_len - 2;
    return with_half_len(K, [&](auto kc) {
        constexpr int KK = decltype(kc)::value;
        AnalysisArgs<KK> a = {};
        a.src = in; a.filt = filter_fwd;
        dwt_extents(filter_len, n0, n1, n2, &a.d0, &a.d1, &a.d2);
        const long long dvol = (long long)a.d0 * a.d1 * a.d2;
        a.band0 = out; a.bandh = out + dvol;
        a.cstride0 = 8 * dvol; a.cstrideh = 8 * dvol;
        a.C = C; a.n0 = n0; a.n1 = n1; a.n2 = n2; a.lo0 = lo; a.lo1 = lo; a.lo2 = lo;
        return launch_analysis<KK>(a, false, taps, (hipStream_t)stream);
    });
}

extern "C" int lfgc_dwt_level_f32(const float* in, const float* filter_fwd, const float* taps, float* out,
                                  int C, int n0, int n1, int n2, lfgc_stream_t stream) {
    return lfgc_dwt_level_len_f32(in, filter_fwd, taps, 4, out, C, n0, n1, n2, stream);
}

// ---- read-only plan queries (include/lfgc.h): the selections above, nothing launched --------------------------------

extern "C" int lfgc_idwt_level_plan(int filter_len, int has_taps, int has_drop, int C, int d0, int d1, int d2,
                                    int t0, int t1, int t2, lfgc_wavelet_plan_info* out) {
    if (!out) return LFGC_E_NULL;
    const int K = half_len(filter_len, has_taps != 0);
    if (!K) return LFGC_E_UNSUPPORTED;
    const int rc = check_level_shape(filter_len, C, d0, d1, d2, t0, t1, t2);
    if (rc != LFGC_OK) return rc;
    lfgc_wavelet_plan_info p;
    const int rs = idwt_select(K, has_taps != 0, has_drop != 0, C, d0, d1, d2, t0, t1, t2, &p);
    if (rs == LFGC_OK) *out = p;
    return rs;
}

extern "C" int lfgc_idwt_level_bwd_plan(int filter_len, int has_taps, int has_drop, int C, int d0, int d1, int d2,
                                        int t0, int t1, int t2, lfgc_wavelet_plan_info* out) {
    if (!out) return LFGC_E_NULL;
    const int K = half_len(filter_len, has_taps != 0);
    if (!K) return LFGC_E_UNSUPPORTED;
    const int rc = check_level_shape(filter_len, C, d0, d1, d2, t0, t1, t2);
    if (rc != LFGC_OK) return rc;
    lfgc_wavelet_plan_info p;
    const int rs = analysis_select(K, has_taps != 0, has_drop != 0, C, t0, t1, t2, d0, d1, d2, &p);
    if (rs == LFGC_OK) *out = p;
    return rs;
}

extern "C" int lfgc_dwt_level_plan(int filter_len, int has_taps, int C, int n0, int n1, int n2, lfgc_wavelet_plan_info* out) {
    if (!out) return LFGC_E_NULL;
    const int K = half_len(filter_len, has_taps != 0);
    if (!K) return LFGC_E_UNSUPPORTED;
    if (C < 1 || n0 < 1 || n1 < 1 || n2 < 1) return LFGC_E_SHAPE;
    int d0, d1, d2;
    dwt_extents(filter_len, n0, n1, n2, &d0, &d1, &d2);
    lfgc_wavelet_plan_info p;
    const int rs = analysis_select(K, has_taps != 0, false, C, n0, n1, n2, d0, d1, d2, &p);
    if (rs == LFGC_OK) *out = p;
    return rs;
}

extern "C" int lfgc_grid_layout_f32(const float* src, float* dst, int C, int64_t voxels, int channel_stride,
                                    int to_channel_last, lfgc_stream_t stream) {
    if (!src || !dst) return LFGC_E_NULL;
    if (C < 1 || voxels < 1 || channel_stride < C) return LFGC_E_SHAPE;
    const unsigned g = (unsigned)((voxels + 63) / 64);
    if (to_channel_last)
        hipLaunchKernelGGL(first_to_last_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, src, dst, C, (long long)voxels, channel_stride);
    else
        hipLaunchKernelGGL(last_to_first_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, src, dst, C, (long long)voxels, channel_stride);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}
