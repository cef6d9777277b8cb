// lfgc_residual.hip -- the error-bounded residual layer over a decoded volume (gfx950), DESIGN.md 3.6.
// With p the model's fp32 prediction of a voxel, g the ground truth, eps the bound, step = eps + eps and inv = 1.0f / step:
//   t = (g - p) * inv;  q = rintf(t);  escape unless |q| <= 127;  r = p + (float)(int)q * step;
//   escape unless |(double)g - (double)r| <= (double)eps;  symbol = zigzag(q) in 0..254, 255 for an escape
// every operation one fp32 rounding (no fma).  An escape is stored verbatim (the bits of g, in lattice order) and decodes to
// them; every other voxel decodes to r, which the encoder has tested against the bound in double -- so the bound holds at
// every voxel provided the decoder's p has the encoder's bits.  Both sides therefore sum  bits(p_i) * (2 i + 1)  mod 2^64
// over the slab (integer adds: order-free, deterministic) and the caller compares the two sums.
//   lfgc_residual_quantize_f32   p, g -> symbols + checksum       one streaming pass, 9 bytes per voxel
//   lfgc_residual_outliers_f32   symbols, g -> the escapes' g     selection (lfgc_select.h), predicate symbol == 255
//   lfgc_residual_apply_f32      p, symbols, escapes -> volume    the same selection with a sink that writes every voxel
// Nothing allocated, no synchronisation; one writer per output address except the integer atomics of checksum and status.
#include <float.h>
#include "lfgc_select.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;                 // streaming passes: at most 8 workgroups per CU, grid-stride beyond
constexpr unsigned kEscape = 255;

struct Quantiser { float eps, step, inv; };

// The symbol of one voxel (the arithmetic of the header above).
__device__ __forceinline__ unsigned residual_symbol(float p, float g, const Quantiser& s) {
    const float q = rintf(__fmul_rn(__fsub_rn(g, p), s.inv));
    if (!(fabsf(q) <= 127.0f)) return kEscape;                   // NaN, Inf and too large, before any conversion to int
    const int qi = (int)q;
    const float r = __fadd_rn(p, __fmul_rn((float)qi, s.step));
    if (!(fabs((double)g - (double)r) <= (double)s.eps)) return kEscape;
    return (((unsigned)qi << 1) ^ (unsigned)(qi >> 31)) & 0xFFu;
}

// What a symbol below 255 decodes to.
__device__ __forceinline__ float residual_value(float p, unsigned sym, float step) {
    const int qi = (int)(sym >> 1) ^ -(int)(sym & 1u);
    return __fadd_rn(p, __fmul_rn((float)qi, step));
}

__device__ __forceinline__ unsigned long long checksum_term(float p, long long i) {
    return (unsigned long long)__float_as_uint(p) * (2ull * (unsigned long long)i + 1ull);
}

// Per-wave shuffle reduce, per-workgroup partial, one 64-bit integer atomic per workgroup.  Holds a barrier.
__device__ __forceinline__ void checksum_flush(unsigned long long acc, unsigned long long* checksum) {
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    __shared__ unsigned long long s_acc[kBlock / 64];
    if ((threadIdx.x & 63) == 0) s_acc[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(checksum, s_acc[0] + s_acc[1] + s_acc[2] + s_acc[3]);
}

// VEC: a lane takes 4 voxels with one 16-byte load per input and one 4-byte store of symbols (pred, gt 16-byte and sym
// 4-byte aligned), the n % 4 voxels of the tail one per lane; otherwise one voxel per lane throughout.  Each input is read
// once and not again: non-temporal loads.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void residual_quantize_kernel(const float* pred, const float* gt, long long n, const Quantiser s,
                                                                   unsigned char* sym, unsigned long long* checksum) {
    const long long first = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    unsigned long long acc = 0;
    long long done = 0;
    if (VEC) {
        const long long nvec = n >> 2;
        for (long long v = first; v < nvec; v += stride) {
            const f32x4 p = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pred) + v);
            const f32x4 g = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(gt) + v);
            const unsigned s0 = residual_symbol(p.x, g.x, s), s1 = residual_symbol(p.y, g.y, s);
            const unsigned s2 = residual_symbol(p.z, g.z, s), s3 = residual_symbol(p.w, g.w, s);
            acc += checksum_term(p.x, 4 * v) + checksum_term(p.y, 4 * v + 1) + checksum_term(p.z, 4 * v + 2) +
                   checksum_term(p.w, 4 * v + 3);
            reinterpret_cast<unsigned*>(sym)[v] = s0 | s1 << 8 | s2 << 16 | s3 << 24;
        }
        done = nvec << 2;
    }
    for (long long i = done + first; i < n; i += stride) {
        const float p = __builtin_nontemporal_load(pred + i);
        sym[i] = (unsigned char)residual_symbol(p, __builtin_nontemporal_load(gt + i), s);
        acc += checksum_term(p, i);
    }
    checksum_flush(acc, checksum);
}

// The decoder's checksum of its own prediction, taken before the apply pass may overwrite it.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void residual_checksum_kernel(const float* pred, long long n, unsigned long long* checksum) {
    const long long first = (long long)blockIdx.x * kBlock + threadIdx.x, stride = (long long)gridDim.x * kBlock;
    unsigned long long acc = 0;
    long long done = 0;
    if (VEC) {
        const long long nvec = n >> 2;
        for (long long v = first; v < nvec; v += stride) {
            const f32x4 p = reinterpret_cast<const f32x4*>(pred)[v];
            acc += checksum_term(p.x, 4 * v) + checksum_term(p.y, 4 * v + 1) + checksum_term(p.z, 4 * v + 2) +
                   checksum_term(p.w, 4 * v + 3);
        }
        done = nvec << 2;
    }
    for (long long i = done + first; i < n; i += stride) acc += checksum_term(pred[i], i);
    checksum_flush(acc, checksum);
}

// ---- the selections (lfgc_select.h) ----------------------------------------------------------------------------------------
struct EscapedTruth {            // compaction: flag = symbol 255, the item the bits of g (read for flagged voxels only)
    typedef unsigned Item;
    const unsigned char* sym;
    const unsigned* gt_bits;
    __device__ __forceinline__ bool operator()(long long i, long long n, unsigned& bits) const {
        const bool flag = i < n && sym[i] == kEscape;
        bits = flag ? gt_bits[i] : 0u;
        return flag;
    }
};

struct OutlierSink {             // outliers[rank] = bits of g for an escape
    unsigned* outliers;
    __device__ __forceinline__ void operator()(long long, long long, bool flag, long long rank, const unsigned& bits) const {
        if (flag) outliers[rank] = bits;
    }
};

struct SymbolAndPrediction {     // restoration: flag = symbol 255; the item is what a non-escaped voxel decodes from
    struct Item { unsigned sym; float p; };
    const unsigned char* sym;
    const unsigned* pred_bits;       // loaded as the type the sink stores: out may be pred, and the compiler must see that
    __device__ __forceinline__ bool operator()(long long i, long long n, Item& item) const {
        if (i >= n) { item.sym = 0; item.p = 0.0f; return false; }
        item.sym = sym[i];
        item.p = __uint_as_float(pred_bits[i]);
        return item.sym == kEscape;
    }
};

// out[i] = escape ? outliers[rank] : r, every i < n written.  out may be pred: a thread has loaded its 8 voxels of pred (the
// items) before its first store, no other thread touches them, and the checksum pass ran before this launch.
struct RestoreSink {
    const unsigned* outliers;
    long long K;
    float step;
    unsigned* out_bits;
    const long long* total;
    int* status;
    __device__ __forceinline__ void operator()(long long i, long long n, bool flag, long long rank,
                                               const SymbolAndPrediction::Item& item) const {
        if (i >= n) return;
        if (i == 0 && *total != K) atomicOr(status, 1);
        unsigned bits;
        if (!flag) {
            bits = __float_as_uint(residual_value(item.p, item.sym, step));
        } else if (rank < K) {
            bits = outliers[rank];
        } else {                                             // never a load past the K outliers the caller holds
            bits = 0u;
            atomicOr(status, 2);
        }
        out_bits[i] = bits;
    }
};

inline bool usable(float v) { return v >= FLT_MIN && v <= FLT_MAX; }     // positive, normal, finite; false for NaN

// eps -> (eps, step, 1 / step), each a positive normal fp32 number, else false.
inline bool make_quantiser(float eps, Quantiser* s) {
    const float step = eps + eps;
    if (!usable(eps) || !usable(step)) return false;
    const float inv = 1.0f / step;
    if (!usable(inv)) return false;
    *s = Quantiser{eps, step, inv};
    return true;
}

inline unsigned stream_blocks(long long threads) {
    const long long b = (threads + kBlock - 1) / kBlock;
    return (unsigned)(b < kMaxBlocks ? b : kMaxBlocks);
}

inline bool aligned(const void* p, unsigned bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

}  // namespace

extern "C" int lfgc_residual_quantize_f32(const float* pred, const float* gt, int64_t n, float eps, uint8_t* sym, uint64_t* checksum,
                                          lfgc_stream_t stream) {
    if (!pred || !gt || !sym || !checksum) return LFGC_E_NULL;
    Quantiser s;
    if (n < 1 || !make_quantiser(eps, &s)) return LFGC_E_SHAPE;
    if (!aligned(pred, 4) || !aligned(gt, 4) || !aligned(checksum, 8)) return LFGC_E_ALIGN;
    unsigned long long* sum = reinterpret_cast<unsigned long long*>(checksum);
    if (n >= 4 && aligned(pred, 16) && aligned(gt, 16) && aligned(sym, 4))
        hipLaunchKernelGGL(residual_quantize_kernel<true>, dim3(stream_blocks(n >> 2)), dim3(kBlock), 0, (hipStream_t)stream, pred, gt,
                           (long long)n, s, sym, sum);
    else
        hipLaunchKernelGGL(residual_quantize_kernel<false>, dim3(stream_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, pred, gt,
                           (long long)n, s, sym, sum);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int64_t lfgc_residual_workspace_bytes(int64_t n) { return lfgc_select_workspace(n); }

extern "C" int lfgc_residual_outliers_f32(const uint8_t* sym, const float* gt, int64_t n, float* outliers, int64_t* count,
                                          void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!sym || !gt || !outliers || !count || !workspace) return LFGC_E_NULL;
    if (n < 1) return LFGC_E_SHAPE;
    if (!aligned(gt, 4) || !aligned(outliers, 4) || !aligned(count, 8) || !aligned(workspace, 8)) return LFGC_E_ALIGN;
    return lfgc_select(EscapedTruth{sym, reinterpret_cast<const unsigned*>(gt)}, OutlierSink{reinterpret_cast<unsigned*>(outliers)}, n,
                       reinterpret_cast<long long*>(count), workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int lfgc_residual_apply_f32(const float* pred, const uint8_t* sym, int64_t n, float eps, const float* outliers, int64_t K,
                                       float* out, uint64_t* checksum, int64_t* n_escape, int32_t* status, void* workspace,
                                       int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!pred || !sym || !out || !checksum || !n_escape || !status || !workspace || (K > 0 && !outliers)) return LFGC_E_NULL;
    Quantiser s;
    if (n < 1 || K < 0 || K > n || !make_quantiser(eps, &s)) return LFGC_E_SHAPE;
    if (!aligned(pred, 4) || !aligned(out, 4) || !aligned(outliers, 4) || !aligned(checksum, 8) || !aligned(n_escape, 8) ||
        !aligned(status, 4) || !aligned(workspace, 8))
        return LFGC_E_ALIGN;
    if (workspace_bytes < lfgc_select_workspace(n)) return LFGC_E_WORKSPACE;
    unsigned long long* sum = reinterpret_cast<unsigned long long*>(checksum);
    if (n >= 4 && aligned(pred, 16))
        hipLaunchKernelGGL(residual_checksum_kernel<true>, dim3(stream_blocks(n >> 2)), dim3(kBlock), 0, (hipStream_t)stream, pred,
                           (long long)n, sum);
    else
        hipLaunchKernelGGL(residual_checksum_kernel<false>, dim3(stream_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, pred,
                           (long long)n, sum);
    LFGC_HIP_CHECK_LAUNCH();
    const long long* total = reinterpret_cast<const long long*>(n_escape);
    return lfgc_select(SymbolAndPrediction{sym, reinterpret_cast<const unsigned*>(pred)},
                       RestoreSink{reinterpret_cast<const unsigned*>(outliers), (long long)K, s.step, reinterpret_cast<unsigned*>(out), total,
                                   status},
                       n, reinterpret_cast<long long*>(n_escape), workspace, workspace_bytes, (hipStream_t)stream);
}
