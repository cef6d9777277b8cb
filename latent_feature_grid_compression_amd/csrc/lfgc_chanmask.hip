// lfgc_chanmask.hip -- the per-cell ("channel-shared") form of the checkpoint codec's pruning mask (gfx950), DESIGN.md 3.6.
// A coefficient tensor is x[c][j], c < C channels, j < S cells; every drop layer multiplies it by one factor per CELL, so a
// pruned model's zero pattern repeats in all C channels.  Mode 2 of the mask file stores it once:
//   lfgc_codec_support_f32          flags[j] = any_c x[c][j] != 0                        the one pass over the whole tensor
//   lfgc_codec_pack_flags_u8        flag bytes -> MSB-first bits
//   lfgc_codec_compact_support_f32  V[c][r] = x[c][j_r], j_r the r-th flagged cell       selection over the S cells
//   lfgc_codec_expand_support_f32   out[c][j] = support bit j ? V[c][rank j] : 0         its inverse
// Integer and copy work only: bit-exact by construction, one writer per output address, no atomics, nothing allocated, no
// synchronisation.  The two selections are lfgc_select (count / scan / write) with the sinks below.
#include "lfgc_select.h"

namespace {

constexpr int kBlock = 256;
constexpr int kInFlight = 8;                     // channel rows a lane has outstanding in the support pass

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- support: OR over the channels ----------------------------------------------------------------------------------------
// Lanes run over consecutive cells, so each channel's row is one coalesced stream; the tensor is read exactly once, with
// non-temporal loads, kInFlight rows ahead of their use.  VEC: thread = 4 cells, one 16-byte load per channel (S % 4 == 0
// keeps every row 16-byte aligned when x is) and one 4-byte store of the four flags.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void support_kernel(const float* __restrict__ x, int C, long long S,
                                                         unsigned char* __restrict__ flags) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (VEC) {
        const long long j = t * 4;
        if (j >= S) return;
        const f32x4* row = reinterpret_cast<const f32x4*>(x + j);
        const long long stride = S >> 2;
        bool a0 = false, a1 = false, a2 = false, a3 = false;
        int c = 0;
        for (; c + kInFlight <= C; c += kInFlight) {
            f32x4 v[kInFlight];
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) v[k] = __builtin_nontemporal_load(row + (c + k) * stride);
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) {
                a0 |= v[k].x != 0.0f; a1 |= v[k].y != 0.0f; a2 |= v[k].z != 0.0f; a3 |= v[k].w != 0.0f;
            }
        }
        for (; c < C; ++c) {
            const f32x4 v = __builtin_nontemporal_load(row + c * stride);
            a0 |= v.x != 0.0f; a1 |= v.y != 0.0f; a2 |= v.z != 0.0f; a3 |= v.w != 0.0f;
        }
        *reinterpret_cast<unsigned*>(flags + j) = (unsigned)a0 | (unsigned)a1 << 8 | (unsigned)a2 << 16 | (unsigned)a3 << 24;
    } else {
        if (t >= S) return;
        const float* row = x + t;
        bool a = false;
        int c = 0;
        for (; c + kInFlight <= C; c += kInFlight) {
            float v[kInFlight];
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) v[k] = __builtin_nontemporal_load(row + (c + k) * S);
#pragma unroll
            for (int k = 0; k < kInFlight; ++k) a |= v[k] != 0.0f;
        }
        for (; c < C; ++c) a |= __builtin_nontemporal_load(row + c * S) != 0.0f;
        flags[t] = (unsigned char)a;
    }
}

// ---- flag bytes -> bits: thread = one output byte = 8 flags (one 8-byte load when whole and aligned) -------------------------
__global__ __launch_bounds__(kBlock) void pack_flags_kernel(const unsigned char* __restrict__ flags, long long n,
                                                            unsigned char* __restrict__ bits, long long nbytes, bool aligned) {
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nbytes) return;
    unsigned b = 0;
    if (aligned && j * 8 + 8 <= n) {
        const unsigned long long w = *reinterpret_cast<const unsigned long long*>(flags + j * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) b |= (unsigned)(((w >> (8 * k)) & 0xFFull) != 0) << (7 - k);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long i = j * 8 + k;
            b |= (unsigned)(i < n && flags[i] != 0) << (7 - k);
        }
    }
    bits[j] = (unsigned char)b;
}

// ---- the selections over the S cells (lfgc_select.h) -----------------------------------------------------------------------
struct FlagByte {                // compaction: flag = flags[j] != 0
    struct Item {};
    const unsigned char* flags;
    __device__ __forceinline__ bool operator()(long long i, long long n, Item&) const { return i < n && flags[i] != 0; }
};

struct SupportBit {              // expansion: flag = bit (bit_offset + j) of the support stream, MSB first
    struct Item {};
    const unsigned char* support;
    long long bit_offset;
    __device__ __forceinline__ bool operator()(long long i, long long n, Item&) const {
        if (i >= n) return false;
        const long long b = bit_offset + i;
        return (support[b >> 3] >> (7 - (int)(b & 7))) & 1;
    }
};

struct SupportCompactSink {      // V[c * K + rank] = x[c * S + j] for a flagged cell j; K = the scanned total
    const float* x;
    float* V;
    int C;
    long long S;
    const long long* total;
    __device__ __forceinline__ void operator()(long long i, long long, bool flag, long long rank, const FlagByte::Item&) const {
        if (!flag) return;
        const long long K = *total;              // rank < K <= S: every store lies inside V[0, C * K)
#pragma unroll 4
        for (int c = 0; c < C; ++c) V[c * K + rank] = x[c * S + i];
    }
};

struct SupportExpandSink {       // out[c * S + j] = flagged ? V[c * K + rank] : 0, every j < S written for every channel
    const float* V;
    float* out;
    int C;
    long long S, K;
    const long long* total;
    int* status;
    __device__ __forceinline__ void operator()(long long i, long long n, bool flag, long long rank, const SupportBit::Item&) const {
        if (i >= n) return;
        if (i == 0 && *total != K) *status |= 1;         // one thread of the launch: a single writer
        const long long last = (long long)C * K - 1;     // every index into V is clamped to it; K = 0: nothing is loaded
        const bool load = flag && last >= 0;
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            long long idx = c * K + rank;
            if (idx > last) idx = last;
            out[c * S + i] = load ? V[idx] : 0.0f;
        }
    }
};

inline bool grid_ok(long long blocks) { return blocks <= 0x7fffffffLL; }

}  // namespace

extern "C" int lfgc_codec_support_f32(const float* x, int C, int64_t S, uint8_t* flags, lfgc_stream_t stream) {
    if (!x || !flags) return LFGC_E_NULL;
    if (C < 1 || S < 1 || S > INT64_MAX / C) return LFGC_E_SHAPE;
    const bool vec = (S & 3) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)flags & 3) == 0;
    const long long threads = vec ? S >> 2 : S;
    const long long blocks = (threads + kBlock - 1) / kBlock;
    if (!grid_ok(blocks)) return LFGC_E_UNSUPPORTED;
    if (vec)
        hipLaunchKernelGGL(support_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, x, C, (long long)S, flags);
    else
        hipLaunchKernelGGL(support_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, x, C, (long long)S, flags);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_codec_pack_flags_u8(const uint8_t* flags, int64_t n, uint8_t* bits, lfgc_stream_t stream) {
    if (!flags || !bits) return LFGC_E_NULL;
    if (n < 1) return LFGC_E_SHAPE;
    const long long nbytes = (n + 7) / 8;
    const long long blocks = (nbytes + kBlock - 1) / kBlock;
    if (!grid_ok(blocks)) return LFGC_E_UNSUPPORTED;
    hipLaunchKernelGGL(pack_flags_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, flags, (long long)n, bits,
                       nbytes, ((uintptr_t)flags & 7) == 0);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_codec_compact_support_f32(const float* x, int C, int64_t S, const uint8_t* flags, float* V, int64_t* count,
                                              void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!x || !flags || !V || !count || !workspace) return LFGC_E_NULL;
    if (C < 1 || S < 1 || S > INT64_MAX / C) return LFGC_E_SHAPE;
    const long long* total = reinterpret_cast<const long long*>(count);
    return lfgc_select(FlagByte{flags}, SupportCompactSink{x, V, C, (long long)S, total}, S, reinterpret_cast<long long*>(count),
                       workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int lfgc_codec_expand_support_f32(const uint8_t* support, int64_t bit_offset, int C, int64_t S, const float* V, int64_t K,
                                             float* out, int32_t* status, void* workspace, int64_t workspace_bytes,
                                             lfgc_stream_t stream) {
    if (!support || !V || !out || !status || !workspace) return LFGC_E_NULL;
    if (C < 1 || S < 1 || S > INT64_MAX / C || bit_offset < 0 || K < 0 || K > S) return LFGC_E_SHAPE;
    LfgcSelectWorkspace w;
    if (workspace_bytes < lfgc_select_workspace(S, workspace, &w)) return LFGC_E_WORKSPACE;
    return lfgc_select(SupportBit{support, bit_offset}, SupportExpandSink{V, out, C, (long long)S, (long long)K, w.offsets + w.nblocks, status},
                       S, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}
