// lfgc_codec.hip -- device side of the binary checkpoint codec (gfx950): the per-coefficient work of the reference's
// store_model_parameters / restore_model (model/model_utils.py:120-332), which there is Python string and list code
// (O(n^2) mask concatenation :207-208, np.insert per pruned element :302-305, scikit-learn k-means on the host).
//   lfgc_codec_mask_f32        bit mask of the non-zero coefficients, MSB first (:204-208, binary_writing :89-107)
//   lfgc_codec_compact_f32     order-preserving removal of the zeros (:210-212)
//   lfgc_codec_kmeans1d_f32    2^bits-entry codebook of a 1-D value set by Lloyd iterations + labels (:65-70, :176-186)
//   lfgc_codec_kmeans1d_sorted_f32 / lfgc_codec_labels_u16_f32   the same for up to 2^16 entries, over sorted values
//   lfgc_codec_pack_labels     labels -> `bits`-wide MSB-first byte stream (ints_to_bits_to_bytes :79-90, tail left-aligned)
//   lfgc_codec_dequant_f32     labels (`bits` wide, MSB first) -> codebook values (read_in_data_quantized :255-275)
//   lfgc_codec_expand_f32      re-insertion of the zeros by the mask (:297-306)
// Byte / index work, bound by HBM: every kernel streams its input once with coalesced rows; prefix sums are
// block-count + single-block scan + rank-in-block from wave ballots (lfgc_select.h).  Integer results are bit-exact by
// construction.
#include "lfgc_select.h"

namespace {

constexpr int kBlock = 256;

// ---- mask -----------------------------------------------------------------------------------------------------------
// thread = one output byte = 8 consecutive coefficients (two 16-byte loads when aligned)
__global__ __launch_bounds__(kBlock) void mask_kernel(const float* __restrict__ x, long long n, unsigned char* __restrict__ mask,
                                                      long long nbytes) {
    const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (j >= nbytes) return;
    unsigned b = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long long i = j * 8 + k;
        const float v = i < n ? x[i] : 0.0f;
        b |= (unsigned)(v != 0.0f) << (7 - k);
    }
    mask[j] = (unsigned char)b;
}

// ---- order-preserving selection (lfgc_select.h): the codec's predicates and sinks ----------------------------------------
struct NonZero {                 // compaction: flag = x[i] != 0, the item is the value
    typedef float Item;
    const float* x;
    __device__ __forceinline__ bool operator()(long long i, long long n, float& v) const {
        v = i < n ? x[i] : 0.0f;
        return v != 0.0f;
    }
};

struct MaskBit {                 // expansion: flag = bit (bit_offset + i) of the mask, MSB first
    struct Item {};
    const unsigned char* mask;
    long long bit_offset;
    __device__ __forceinline__ bool operator()(long long i, long long n, Item&) const {
        if (i >= n) return false;
        const long long b = bit_offset + i;
        return (mask[b >> 3] >> (7 - (int)(b & 7))) & 1;
    }
};

struct CompactSink {             // out[rank] = x[i] for flagged i
    float* out;
    __device__ __forceinline__ void operator()(long long, long long, bool flag, long long rank, const float& v) const {
        if (flag) out[rank] = v;
    }
};

struct ExpandSink {              // out[i] = flagged ? values[rank] : 0, every i < n written
    const float* values;
    float* out;
    __device__ __forceinline__ void operator()(long long i, long long n, bool flag, long long rank, const MaskBit::Item&) const {
        if (i < n) out[i] = flag ? values[rank] : 0.0f;
    }
};

// ---- 1-D k-means --------------------------------------------------------------------------------------------------------
// centres are kept sorted: a value belongs to the interval between the midpoints of neighbouring centres, found by
// binary search over the k-1 midpoints in LDS; means of intervals stay ordered, so no re-sort is ever needed.
__device__ __forceinline__ int nearest_centre(const float* s_mid, int k, float v) {
    int lo = 0, hi = k - 1;                      // label = number of midpoints < v
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (s_mid[m] < v) lo = m + 1; else hi = m;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void kmeans_accumulate_kernel(const float* __restrict__ x, long long n, int k,
                                                                   const float* __restrict__ centres,
                                                                   double* __restrict__ part_sum, unsigned* __restrict__ part_cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    double* s_sum = reinterpret_cast<double*>(s_raw);                 // k
    unsigned* s_cnt = reinterpret_cast<unsigned*>(s_sum + k);         // k
    float* s_mid = reinterpret_cast<float*>(s_cnt + k);               // k (k-1 used)
    for (int j = threadIdx.x; j < k; j += kBlock) {
        s_sum[j] = 0.0; s_cnt[j] = 0u;
        s_mid[j] = j + 1 < k ? 0.5f * (centres[j] + centres[j + 1]) : 3.4e38f;
    }
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const float v = x[i];
        const int c = nearest_centre(s_mid, k, v);
        atomicAdd(&s_sum[c], (double)v);
        atomicAdd(&s_cnt[c], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += kBlock) {
        part_sum[(long long)blockIdx.x * k + j] = s_sum[j];
        part_cnt[(long long)blockIdx.x * k + j] = s_cnt[j];
    }
}

__global__ __launch_bounds__(kBlock) void kmeans_update_kernel(int k, int nparts, const double* __restrict__ part_sum,
                                                               const unsigned* __restrict__ part_cnt, float* __restrict__ centres) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= k) return;
    double s = 0.0;
    unsigned long long c = 0;
    for (int p = 0; p < nparts; ++p) { s += part_sum[(long long)p * k + j]; c += part_cnt[(long long)p * k + j]; }
    if (c > 0) centres[j] = (float)(s / (double)c);        // an empty cluster keeps its centre
}

__global__ __launch_bounds__(kBlock) void kmeans_label_kernel(const float* __restrict__ x, long long n, int k,
                                                              const float* __restrict__ centres, unsigned char* __restrict__ labels) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    float* s_mid = reinterpret_cast<float*>(s_raw);
    for (int j = threadIdx.x; j < k; j += kBlock) s_mid[j] = j + 1 < k ? 0.5f * (centres[j] + centres[j + 1]) : 3.4e38f;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock)
        labels[i] = (unsigned char)nearest_centre(s_mid, k, x[i]);
}

// ---- 1-D k-means over SORTED values, up to 65 536 centres ------------------------------------------------------------------
// The same Lloyd iteration as above (fp32 midpoints, label = number of midpoints < v, fp64 sums), but in sorted order a
// cluster is the contiguous range [bound[j], bound[j+1]): no histogram, no atomics, no LDS.
constexpr int kSumBlock = 1024;                 // sorted values per precomputed fp64 block sum

// Midpoint of two sorted centres.  Between neighbouring floats a < b the sum rounds, and half the time 0.5f * (a + b) is b
// itself: b would then be labelled a, and a codebook with one centre per value (more centres than values: every small
// tensor at 16 bits) would not reproduce them.  Such a midpoint is moved one float down, so a centre always owns its value.
__device__ __forceinline__ float wide_midpoint(float c0, float c1) {
    const float mid = 0.5f * (c0 + c1);
    return (mid < c1 || !(c0 < c1)) ? mid : nextafterf(c1, c0);
}

__device__ __forceinline__ double wave_sum(double s) {               // fixed-shape butterfly: every lane gets the total
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// wave w of the grid: bsum[w] = fp64 sum of xs[w * 1024, min(n, (w + 1) * 1024))
__global__ __launch_bounds__(kBlock) void sorted_block_sums_kernel(const float* __restrict__ xs, long long n, long long nblocks,
                                                                   double* __restrict__ bsum) {
    const long long w = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (w >= nblocks) return;
    const int lane = threadIdx.x & 63;
    const long long base = w * kSumBlock;
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < kSumBlock / 64; ++t) {
        const long long i = base + t * 64 + lane;
        if (i < n) s += (double)xs[i];
    }
    s = wave_sum(s);
    if (lane == 0) bsum[w] = s;
}

// thread j (0..k): bound[j] = first sorted index of cluster j; bound[0] = 0, bound[k] = n, otherwise the number of values
// <= midpoint j-1 (a value's label is the number of midpoints < it, so cluster j-1 ends where the values exceed it)
__global__ __launch_bounds__(kBlock) void sorted_bounds_kernel(const float* __restrict__ xs, long long n, int k,
                                                               const float* __restrict__ centres, long long* __restrict__ bound) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j > k) return;
    long long lo = 0, hi = n;
    if (j == k) lo = n;
    else if (j == 0) hi = 0;
    else {
        const float mid = wide_midpoint(centres[j - 1], centres[j]);
        while (lo < hi) {                                        // first index whose value is > mid
            const long long m = lo + ((hi - lo) >> 1);
            if (xs[m] <= mid) lo = m + 1; else hi = m;
        }
    }
    bound[j] = lo;
}

// wave j: centre j = mean of xs[bound[j], bound[j+1]): head piece up to the next multiple of 1024, whole blocks from bsum,
// tail piece -- lanes stride over each, then one butterfly.  No prefix-sum differences (cancellation).
__global__ __launch_bounds__(kBlock) void sorted_update_kernel(const float* __restrict__ xs, int k, const long long* __restrict__ bound,
                                                               const double* __restrict__ bsum, float* __restrict__ centres) {
    const int j = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (j >= k) return;
    const int lane = threadIdx.x & 63;
    const long long lo = bound[j], hi = bound[j + 1];
    if (hi <= lo) return;                                        // an empty cluster keeps its centre
    const long long b_lo = (lo + kSumBlock - 1) / kSumBlock;     // first whole block
    const long long b_hi = hi / kSumBlock;                       // one past the last whole block
    double s = 0.0;
    if (b_lo >= b_hi) {                                          // no whole block inside: the range itself
        for (long long i = lo + lane; i < hi; i += 64) s += (double)xs[i];
    } else {
        for (long long i = lo + lane; i < b_lo * kSumBlock; i += 64) s += (double)xs[i];
        for (long long b = b_lo + lane; b < b_hi; b += 64) s += bsum[b];
        for (long long i = b_hi * kSumBlock + lane; i < hi; i += 64) s += (double)xs[i];
    }
    s = wave_sum(s);
    if (lane == 0) centres[j] = (float)(s / (double)(hi - lo));
}

// labels of UNSORTED values against up to 65 536 centres.  LDS holds every (1 << shift)-th midpoint: coarse[t] = midpoint
// ((t + 1) << shift) - 1; t = number of coarse entries < v puts the label in [t << shift, (t << shift) + (1 << shift) - 1],
// searched over the centres themselves (L2).  shift = 0: the table is all midpoints and the second search is empty.
__global__ __launch_bounds__(kBlock) void label_u16_kernel(const float* __restrict__ x, long long n, int k, int shift,
                                                           const float* __restrict__ centres, unsigned short* __restrict__ labels) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    float* s_coarse = reinterpret_cast<float*>(s_raw);
    const int nc = (k - 1) >> shift;
    for (int t = threadIdx.x; t < nc; t += kBlock) {
        const int m = ((t + 1) << shift) - 1;                    // <= k - 2
        s_coarse[t] = wide_midpoint(centres[m], centres[m + 1]);
    }
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        const float v = x[i];
        int lo = 0, hi = nc;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (s_coarse[m] < v) lo = m + 1; else hi = m;
        }
        lo <<= shift;
        hi = lo + (1 << shift) - 1;
        if (hi > k - 1) hi = k - 1;
        while (lo < hi) {                                        // midpoints lo .. hi-1 exist: hi <= k - 1
            const int m = (lo + hi) >> 1;
            if (wide_midpoint(centres[m], centres[m + 1]) < v) lo = m + 1; else hi = m;
        }
        labels[i] = (unsigned short)lo;
    }
}

// ---- label packing -----------------------------------------------------------------------------------------------------------
// thread = one output byte b = stream bits [8b, 8b+8); label i occupies bits [i*bits, (i+1)*bits), MSB first.  At most 8
// labels overlap a byte; bits past n*bits stay zero (left-aligned tail).  Every offset is 64-bit.
template <typename L>
__global__ __launch_bounds__(kBlock) void pack_labels_kernel(const L* __restrict__ labels, long long n, int bits,
                                                             unsigned char* __restrict__ packed, long long nbytes) {
    const long long b = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (b >= nbytes) return;
    const long long bit0 = b * 8;
    const long long first = bit0 / bits;
    long long last = (bit0 + 7) / bits;
    if (last > n - 1) last = n - 1;
    const unsigned mask = (1u << bits) - 1u;
    unsigned out = 0;
    for (long long i = first; i <= last; ++i) {
        const unsigned lab = (unsigned)labels[i] & mask;
        const int shift = (int)((i + 1) * bits - (bit0 + 8));   // label bits below the byte's last bit: -7 .. 15
        out |= shift >= 0 ? lab >> shift : lab << -shift;
    }
    packed[b] = (unsigned char)out;
}

// ---- dequantisation -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void dequant_kernel(const unsigned char* __restrict__ packed, long long packed_bytes,
                                                         int bits, long long n, const float* __restrict__ centres,
                                                         float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    unsigned label;
    if (bits == 8) {
        label = packed[i];
    } else {                                     // bits [bits*i, bits*(i+1)) of the stream, MSB first (<= 16 bits: 3 bytes)
        const long long b0 = i * bits;
        const long long byte0 = b0 >> 3;
        unsigned w = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) w = (w << 8) | (byte0 + k < packed_bytes ? packed[byte0 + k] : 0u);
        label = (w >> (24 - (int)(b0 & 7) - bits)) & ((1u << bits) - 1u);
    }
    out[i] = centres[label];
}

inline unsigned blocks_cap(long long n, int per, long long cap) {
    long long g = (n + per - 1) / per;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int lfgc_codec_mask_f32(const float* x, int64_t n, uint8_t* mask, lfgc_stream_t stream) {
    if (!x || !mask) return LFGC_E_NULL;
    if (n < 1) return LFGC_E_SHAPE;
    const long long nbytes = (n + 7) / 8;
    hipLaunchKernelGGL(mask_kernel, dim3((unsigned)((nbytes + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       x, (long long)n, mask, nbytes);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int64_t lfgc_codec_select_workspace_bytes(int64_t n) { return lfgc_select_workspace(n); }

extern "C" int lfgc_codec_compact_f32(const float* x, int64_t n, float* out, int64_t* count, void* workspace,
                                      int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!x || !out || !count || !workspace) return LFGC_E_NULL;
    if (n < 1) return LFGC_E_SHAPE;
    return lfgc_select(NonZero{x}, CompactSink{out}, n, reinterpret_cast<long long*>(count), workspace, workspace_bytes,
                       (hipStream_t)stream);
}

extern "C" int lfgc_codec_expand_f32(const uint8_t* mask, int64_t bit_offset, int64_t n, const float* values, float* out,
                                     void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!mask || !values || !out || !workspace) return LFGC_E_NULL;
    if (n < 1 || bit_offset < 0) return LFGC_E_SHAPE;
    return lfgc_select(MaskBit{mask, bit_offset}, ExpandSink{values, out}, n, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int64_t lfgc_codec_kmeans_workspace_bytes(int k) {
    if (k < 1) return 0;
    return (int64_t)LFGC_CODEC_KMEANS_PARTS * k * (8 + 4) + 64;
}

extern "C" int lfgc_codec_kmeans1d_f32(const float* x, int64_t n, int k, float* centres, uint8_t* labels, int iterations,
                                       void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!x || !centres || !workspace) return LFGC_E_NULL;
    if (n < 1 || k < 1 || k > 256 || iterations < 0) return LFGC_E_SHAPE;
    if (workspace_bytes < lfgc_codec_kmeans_workspace_bytes(k)) return LFGC_E_WORKSPACE;
    const unsigned parts = blocks_cap(n, kBlock * 8, LFGC_CODEC_KMEANS_PARTS);
    double* part_sum = reinterpret_cast<double*>(workspace);
    unsigned* part_cnt = reinterpret_cast<unsigned*>(part_sum + (size_t)LFGC_CODEC_KMEANS_PARTS * k);
    const int lds = k * (8 + 4 + 4);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(kmeans_accumulate_kernel, dim3(parts), dim3(kBlock), lds, (hipStream_t)stream,
                           x, (long long)n, k, centres, part_sum, part_cnt);
        LFGC_HIP_CHECK_LAUNCH();
        hipLaunchKernelGGL(kmeans_update_kernel, dim3((k + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream,
                           k, (int)parts, part_sum, part_cnt, centres);
        LFGC_HIP_CHECK_LAUNCH();
    }
    if (labels) {
        hipLaunchKernelGGL(kmeans_label_kernel, dim3(blocks_cap(n, kBlock * 4, 4096)), dim3(kBlock), k * 4, (hipStream_t)stream,
                           x, (long long)n, k, centres, labels);
        LFGC_HIP_CHECK_LAUNCH();
    }
    return LFGC_OK;
}

extern "C" int64_t lfgc_codec_kmeans_sorted_workspace_bytes(int64_t n, int k) {
    if (n < 1 || k < 1 || k > LFGC_CODEC_KMEANS_MAX_K) return 0;
    const int64_t nblocks = (n + kSumBlock - 1) / kSumBlock;
    return nblocks * 8 + ((int64_t)k + 1) * 8 + 64;
}

extern "C" int lfgc_codec_kmeans1d_sorted_f32(const float* x_sorted, int64_t n, int k, float* centres, int iterations,
                                              void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!x_sorted || !centres || !workspace) return LFGC_E_NULL;
    if (n < 1 || k < 1 || k > LFGC_CODEC_KMEANS_MAX_K || iterations < 0) return LFGC_E_SHAPE;
    if (workspace_bytes < lfgc_codec_kmeans_sorted_workspace_bytes(n, k)) return LFGC_E_WORKSPACE;
    const long long nblocks = (n + kSumBlock - 1) / kSumBlock;
    const long long sum_grid = (nblocks + kBlock / 64 - 1) / (kBlock / 64);
    if (sum_grid > 0x7fffffffLL) return LFGC_E_UNSUPPORTED;
    double* bsum = reinterpret_cast<double*>(workspace);
    long long* bound = reinterpret_cast<long long*>(bsum + nblocks);
    if (iterations > 0) {
        hipLaunchKernelGGL(sorted_block_sums_kernel, dim3((unsigned)sum_grid), dim3(kBlock), 0, (hipStream_t)stream,
                           x_sorted, (long long)n, nblocks, bsum);
        LFGC_HIP_CHECK_LAUNCH();
    }
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(sorted_bounds_kernel, dim3((unsigned)(k / kBlock + 1)), dim3(kBlock), 0, (hipStream_t)stream,
                           x_sorted, (long long)n, k, centres, bound);
        LFGC_HIP_CHECK_LAUNCH();
        hipLaunchKernelGGL(sorted_update_kernel, dim3((unsigned)((k + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0,
                           (hipStream_t)stream, x_sorted, k, bound, bsum, centres);
        LFGC_HIP_CHECK_LAUNCH();
    }
    return LFGC_OK;
}

extern "C" int lfgc_codec_labels_u16_f32(const float* x, int64_t n, int k, const float* centres, uint16_t* labels,
                                         lfgc_stream_t stream) {
    if (!x || !centres || !labels) return LFGC_E_NULL;
    if (n < 1 || k < 1 || k > LFGC_CODEC_KMEANS_MAX_K) return LFGC_E_SHAPE;
    const int shift = k <= 8192 ? 0 : 8;                         // all midpoints in LDS (<= 32 KB), or every 256th (<= 1 KB)
    hipLaunchKernelGGL(label_u16_kernel, dim3(blocks_cap(n, kBlock * 4, 4096)), dim3(kBlock), ((k - 1) >> shift) * 4,
                       (hipStream_t)stream, x, (long long)n, k, shift, centres, labels);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_codec_pack_labels(const void* labels, int label_bytes, int64_t n, int bits, uint8_t* packed,
                                      int64_t packed_bytes, lfgc_stream_t stream) {
    if (!labels || !packed) return LFGC_E_NULL;
    if (n < 1 || bits < 1 || bits > 16 || (label_bytes != 1 && label_bytes != 2) || (bits > 8 && label_bytes != 2))
        return LFGC_E_SHAPE;
    if (n > INT64_MAX / 16) return LFGC_E_SHAPE;
    const long long nbytes = (n * bits + 7) / 8;
    if (packed_bytes < nbytes) return LFGC_E_SHAPE;
    const long long grid = (nbytes + kBlock - 1) / kBlock;
    if (grid > 0x7fffffffLL) return LFGC_E_UNSUPPORTED;
    if (label_bytes == 1)
        hipLaunchKernelGGL(pack_labels_kernel<unsigned char>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream,
                           reinterpret_cast<const unsigned char*>(labels), (long long)n, bits, packed, nbytes);
    else
        hipLaunchKernelGGL(pack_labels_kernel<unsigned short>, dim3((unsigned)grid), dim3(kBlock), 0, (hipStream_t)stream,
                           reinterpret_cast<const unsigned short*>(labels), (long long)n, bits, packed, nbytes);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_codec_dequant_f32(const uint8_t* packed, int64_t packed_bytes, int bits, int64_t n, const float* centres,
                                      float* out, lfgc_stream_t stream) {
    if (!packed || !centres || !out) return LFGC_E_NULL;
    if (n < 1 || bits < 1 || bits > 16 || packed_bytes * 8 < n * (int64_t)bits) return LFGC_E_SHAPE;
    hipLaunchKernelGGL(dequant_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       packed, (long long)packed_bytes, bits, (long long)n, centres, out);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}
