// lfgc_rans.hip -- lossless entropy stage of the checkpoint codec (gfx950): byte-symbol rANS with a static
// order-0 model, interleaved over the 64 lanes of a wave.  Frequencies sum to 4096, the state is 32 bits in [2^16, 2^32),
// renormalisation moves one 16-bit word, the initial encoder state is 2^16.
//   lfgc_codec_histogram_u8          256 int64 counts of a byte array
//   lfgc_codec_rans_normalize_host   counts -> frequencies (host, integer)
//   lfgc_codec_rans_encode_count     words per chunk, their 64-bit offsets and their total (count + scan of lfgc_select.h)
//   lfgc_codec_rans_encode_write     the whole stream, every chunk straight at its final place
//   lfgc_codec_rans_decode           stream -> bytes, with a status word for a stream that does not decode
// Stream, little-endian:  u32 n | u16 R | u16 0 | u16 f[256] | u32 words[nc]  then per chunk  u32 state[64], u16 word[words[c]],
// nc = ceil(n / 64R).  One wave per chunk; lane l codes the chunk positions 64 r + l, r = 0..R-1; a position >= n is skipped.
// The decoder walks r upwards and the lanes that renormalise in a round take consecutive words in ascending lane order, so
// the encoder walks r downwards and fills the chunk's words from the end.  A chunk may start on any even byte: the stream is
// addressed as 16-bit words throughout.  Integer arithmetic only: every byte is fixed by the format.
#include "lfgc_select.h"
#include <algorithm>

namespace {

constexpr int kRansBlock = 256;                    // 4 waves = 4 chunks per workgroup; also one thread per symbol of the model
constexpr int kRansWaves = kRansBlock / 64;
constexpr int kRansProbBits = 12;
constexpr unsigned kRansLow = 1u << 16;
constexpr int kRansHeaderU16 = 4 + 256;            // n (2), R, 0, f[256]
constexpr int kRansBatch = 8;                      // rounds whose symbols the encoder loads ahead
constexpr int kHistMaxGrid = 1024;
constexpr long long kHistMaxBytes = 1LL << 31;     // bytes per workgroup: its 32-bit counters cannot overflow

enum { kRansOverrun = 1, kRansFinalState = 2, kRansCursor = 4, kRansLayout = 8 };

// ---- histogram ---------------------------------------------------------------------------------------------------------------
// One LDS histogram per wave (a pruned mask is mostly one symbol: four waves on one counter would serialise), flushed with
// 64-bit integer atomics, non-zero bins only.
__global__ __launch_bounds__(kRansBlock) void histogram_u8_kernel(const unsigned char* __restrict__ sym, long long n, long long nvec,
                                                                  unsigned long long* __restrict__ counts) {
    __shared__ unsigned s_hist[kRansWaves][256];
    for (int w = 0; w < kRansWaves; ++w) s_hist[w][threadIdx.x] = 0u;
    __syncthreads();
    unsigned* h = s_hist[threadIdx.x >> 6];
    const long long stride = (long long)gridDim.x * kRansBlock;
    const unsigned* sym4 = reinterpret_cast<const unsigned*>(sym);          // nvec > 0 only for a 4-byte aligned array
    for (long long i = (long long)blockIdx.x * kRansBlock + threadIdx.x; i < nvec; i += stride) {
        const unsigned v = sym4[i];
        atomicAdd(&h[v & 255u], 1u);
        atomicAdd(&h[(v >> 8) & 255u], 1u);
        atomicAdd(&h[(v >> 16) & 255u], 1u);
        atomicAdd(&h[v >> 24], 1u);
    }
    for (long long i = nvec * 4 + (long long)blockIdx.x * kRansBlock + threadIdx.x; i < n; i += stride) atomicAdd(&h[sym[i]], 1u);
    __syncthreads();
    unsigned long long c = 0;
    for (int w = 0; w < kRansWaves; ++w) c += s_hist[w][threadIdx.x];
    if (c) atomicAdd(&counts[threadIdx.x], c);
}

// ---- the model in LDS ----------------------------------------------------------------------------------------------------------
// s_fc[s] = cum[s] | f[s] << 16 (f <= 4096, cum <= 4096).  Holds barriers: every thread of the workgroup calls it.
__device__ __forceinline__ void rans_load_model(const unsigned short* __restrict__ freq, unsigned* s_f, unsigned* s_fc) {
    s_f[threadIdx.x] = freq[threadIdx.x];
    __syncthreads();
    unsigned cum = 0;
    for (int u = 0; u < (int)threadIdx.x; ++u) cum += s_f[u];
    s_fc[threadIdx.x] = (cum & 0xFFFFu) | (s_f[threadIdx.x] << 16);
    __syncthreads();
}

__device__ __forceinline__ int lanes_below(unsigned long long ballot, int lane) {
    return __popcll(ballot & ((1ull << lane) - 1ull));
}

// ---- encoder ---------------------------------------------------------------------------------------------------------------------
// WRITE = false: counts[c] = words of chunk c.  WRITE = true: the same coder again, writing the header, words[nc], and chunk
// c's states and words at 16-bit index 260 + 2 nc + 128 c + offsets[c].  In round r a lane that emits writes at
// cursor - k + (emitting lanes below it), k = emitting lanes of the round, then cursor -= k: one writer per address.  Every
// store is fenced to the chunk's own range and to the buffer, so a frequency table that does not belong to the symbols
// (whatever it then codes) cannot write elsewhere.
template <bool WRITE>
__global__ __launch_bounds__(kRansBlock) void rans_encode_kernel(const unsigned char* __restrict__ sym, long long n, int R, long long nc,
                                                                 const unsigned short* __restrict__ freq, unsigned* __restrict__ counts,
                                                                 const long long* __restrict__ offsets,
                                                                 unsigned short* __restrict__ out, long long out_u16) {
    __shared__ unsigned s_f[256], s_fc[256];
    rans_load_model(freq, s_f, s_fc);
    const int lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * kRansWaves + (threadIdx.x >> 6);
    if (WRITE && blockIdx.x == 0) {                                      // out_u16 >= 260 + 2 nc: checked by the entry
        out[4 + threadIdx.x] = (unsigned short)s_f[threadIdx.x];
        if (threadIdx.x == 0) {
            out[0] = (unsigned short)(n & 0xFFFF);
            out[1] = (unsigned short)((unsigned long long)n >> 16);
            out[2] = (unsigned short)R;
            out[3] = 0;
        }
    }
    if (c >= nc) return;
    const long long base = c * 64 * R;
    long long wbase = 0, wend = 0;
    int cursor = 0;
    if (WRITE) {
        const unsigned nw = counts[c];
        wbase = kRansHeaderU16 + 2 * nc + 128 * c + offsets[c] + 128;
        wend = wbase + nw < out_u16 ? wbase + nw : out_u16;
        cursor = (int)nw;
        if (lane == 0) {
            out[kRansHeaderU16 + 2 * c] = (unsigned short)(nw & 0xFFFFu);
            out[kRansHeaderU16 + 2 * c + 1] = (unsigned short)(nw >> 16);
        }
    }
    unsigned x = kRansLow;
    unsigned total = 0;
    for (int rb = R; rb > 0; rb -= kRansBatch) {                         // rounds rb-1 down to rb-8
        int s[kRansBatch];
#pragma unroll
        for (int j = 0; j < kRansBatch; ++j) {
            const int r = rb - 1 - j;
            const long long pos = base + 64LL * r + lane;
            s[j] = (r >= 0 && pos < n) ? (int)sym[pos] : -1;
        }
#pragma unroll
        for (int j = 0; j < kRansBatch; ++j) {
            const bool active = s[j] >= 0;
            const unsigned fc = s_fc[active ? s[j] : 0];
            const unsigned f = fc >> 16, cum = fc & 0xFFFFu;
            const bool emit = active && (x >> 20) >= f;                  // not x >= f << 20: f may be 4096
            const unsigned long long bal = __ballot(emit);
            const int k = __popcll(bal);
            if (emit) {
                if (WRITE) {
                    const long long p = wbase + cursor - k + lanes_below(bal, lane);
                    if (p >= wbase && p < wend) out[p] = (unsigned short)(x & 0xFFFFu);
                }
                x >>= 16;
            }
            cursor -= k;
            total += (unsigned)k;
            if (active && f) x = ((x / f) << kRansProbBits) + x % f + cum;     // a true integer divide: exact
        }
    }
    if (WRITE) {
        const long long sp = wbase - 128 + 2 * lane;
        if (sp + 1 < out_u16) {
            out[sp] = (unsigned short)(x & 0xFFFFu);
            out[sp + 1] = (unsigned short)(x >> 16);
        }
    } else if (lane == 0) {
        counts[c] = total;
    }
}

// ---- decoder ---------------------------------------------------------------------------------------------------------------------
// The slot -> symbol table (4096 bytes) and f / cum in LDS.  Every word index is clamped to the chunk's own words, and the
// chunk's range to the buffer, before the load; what the clamps caught, a final state other than 2^16 and a cursor that does
// not end at the chunk's end are reported in *status.
__global__ __launch_bounds__(kRansBlock) void rans_decode_kernel(const unsigned short* __restrict__ in, long long in_u16, long long n, int R,
                                                                 long long nc, const long long* __restrict__ offsets,
                                                                 unsigned char* __restrict__ out, int* __restrict__ status) {
    __shared__ unsigned s_f[256], s_fc[256];
    __shared__ unsigned char s_tab[1 << kRansProbBits];
    rans_load_model(in + 4, s_f, s_fc);
    for (int slot = threadIdx.x; slot < (1 << kRansProbBits); slot += kRansBlock) {
        int lo = 0, hi = 255;                // the last symbol with cum <= slot: symbols with f = 0 before it share its cum
        while (lo < hi) {
            const int m = (lo + hi + 1) >> 1;
            if ((s_fc[m] & 0xFFFFu) <= (unsigned)slot) lo = m; else hi = m - 1;
        }
        s_tab[slot] = (unsigned char)lo;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long long c = (long long)blockIdx.x * kRansWaves + (threadIdx.x >> 6);
    if (c >= nc) return;
    int bad = 0;
    const long long sbase = kRansHeaderU16 + 2 * nc + 128 * c + offsets[c];
    const long long wbase = sbase + 128;
    if (wbase > in_u16) {                                                // not even the states are there
        if (lane == 0) atomicOr(status, (int)kRansLayout);
        return;
    }
    long long nw = (long long)in[kRansHeaderU16 + 2 * c] | ((long long)in[kRansHeaderU16 + 2 * c + 1] << 16);
    if (wbase + nw > in_u16) { nw = in_u16 - wbase; bad |= kRansLayout; }
    unsigned x = (unsigned)in[sbase + 2 * lane] | ((unsigned)in[sbase + 2 * lane + 1] << 16);
    const long long base = c * 64 * R;
    long long cursor = 0;
    for (int r = 0; r < R; ++r) {
        const long long pos = base + 64LL * r + lane;
        const bool active = pos < n;
        if (active) {
            const unsigned slot = x & ((1u << kRansProbBits) - 1u);
            const unsigned s = s_tab[slot];
            const unsigned fc = s_fc[s];
            x = (fc >> 16) * (x >> kRansProbBits) + slot - (fc & 0xFFFFu);
            out[pos] = (unsigned char)s;
        }
        const bool need = active && x < kRansLow;
        const unsigned long long bal = __ballot(need);
        if (need) {
            long long idx = cursor + lanes_below(bal, lane);
            if (idx >= nw) { idx = nw - 1; bad |= kRansOverrun; }
            const unsigned w = idx >= 0 ? (unsigned)in[wbase + idx] : 0u;
            x = (x << 16) | w;
        }
        cursor += __popcll(bal);
    }
    if (x != kRansLow) bad |= kRansFinalState;
    if (cursor != nw) bad |= kRansCursor;
    if (bad) atomicOr(status, bad);
}

// offsets[nc + 1] (64-bit) | counts[nc]
struct RansWorkspace {
    long long nc;
    long long* offsets;
    unsigned* counts;
};

inline bool rans_shape_ok(long long n, int rounds) { return n >= 1 && n <= 0xFFFFFFFFLL && rounds >= 1 && rounds <= 0xFFFF; }

inline long long rans_workspace(long long n, int rounds, void* base, RansWorkspace* w) {
    const long long per = 64LL * rounds;
    const long long nc = (n + per - 1) / per;
    if (w) {
        w->nc = nc;
        w->offsets = reinterpret_cast<long long*>(base);
        w->counts = reinterpret_cast<unsigned*>(w->offsets + nc + 1);
    }
    return (nc + 1) * 8 + nc * 4 + 16;
}

inline unsigned rans_grid(long long nc) { return (unsigned)((nc + kRansWaves - 1) / kRansWaves); }

}  // namespace

extern "C" int lfgc_codec_histogram_u8(const uint8_t* sym, int64_t n, int64_t* counts, lfgc_stream_t stream) {
    if (!sym || !counts) return LFGC_E_NULL;
    if (n < 0) return LFGC_E_SHAPE;
    if ((uintptr_t)counts & 7) return LFGC_E_ALIGN;
    if (n == 0) return LFGC_OK;
    const long long nvec = ((uintptr_t)sym & 3) ? 0 : n / 4;
    const long long blocks = (n + kRansBlock * 16 - 1) / (kRansBlock * 16);
    long long grid = blocks < kHistMaxGrid ? blocks : kHistMaxGrid;
    const long long least = (n + kHistMaxBytes - 1) / kHistMaxBytes;
    if (grid < least) grid = least;
    if (grid > 0x7fffffffLL) return LFGC_E_UNSUPPORTED;
    hipLaunchKernelGGL(histogram_u8_kernel, dim3((unsigned)grid), dim3(kRansBlock), 0, (hipStream_t)stream, sym, (long long)n, nvec,
                       reinterpret_cast<unsigned long long*>(counts));
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_codec_rans_normalize_host(const int64_t* counts, uint16_t* freq) {
    if (!counts || !freq) return LFGC_E_NULL;
    int64_t n = 0;
    for (int s = 0; s < 256; ++s) {
        if (counts[s] < 0 || counts[s] > ((int64_t)1 << 50) || n + counts[s] > ((int64_t)1 << 50)) return LFGC_E_SHAPE;
        n += counts[s];
    }
    if (n == 0) return LFGC_E_SHAPE;
    int64_t f[256], d = 1 << kRansProbBits;
    int order[256];
    for (int s = 0; s < 256; ++s) {
        f[s] = counts[s] == 0 ? 0 : std::max<int64_t>(1, counts[s] * (1 << kRansProbBits) / n);
        d -= f[s];
        order[s] = s;
    }
    std::stable_sort(order, order + 256, [&](int a, int b) { return counts[a] > counts[b]; });   // ties: ascending symbol
    while (d != 0) {
        for (int i = 0; i < 256 && d != 0; ++i) {
            const int s = order[i];
            if (d > 0 && counts[s] > 0) { ++f[s]; --d; }
            else if (d < 0 && f[s] > 1) { --f[s]; ++d; }
        }
    }
    for (int s = 0; s < 256; ++s) freq[s] = (uint16_t)f[s];
    return LFGC_OK;
}

extern "C" int64_t lfgc_codec_rans_workspace_bytes(int64_t n, int rounds) {
    return rans_shape_ok(n, rounds) ? rans_workspace(n, rounds, nullptr, nullptr) : 0;
}

extern "C" int lfgc_codec_rans_encode_count(const uint8_t* sym, int64_t n, int rounds, const uint16_t* freq, int64_t* total_words,
                                            void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!sym || !freq || !total_words || !workspace) return LFGC_E_NULL;
    if (!rans_shape_ok(n, rounds)) return LFGC_E_SHAPE;
    if (((uintptr_t)workspace & 7) || ((uintptr_t)freq & 1) || ((uintptr_t)total_words & 7)) return LFGC_E_ALIGN;
    RansWorkspace w;
    if (workspace_bytes < rans_workspace(n, rounds, workspace, &w)) return LFGC_E_WORKSPACE;
    hipLaunchKernelGGL(rans_encode_kernel<false>, dim3(rans_grid(w.nc)), dim3(kRansBlock), 0, (hipStream_t)stream, sym, (long long)n,
                       rounds, w.nc, freq, w.counts, (const long long*)nullptr, (unsigned short*)nullptr, 0LL);
    LFGC_HIP_CHECK_LAUNCH();
    LfgcScanTotals totals = {{reinterpret_cast<long long*>(total_words), nullptr}};
    return lfgc_select_scan(w.counts, w.offsets, w.nc, 1, totals, (hipStream_t)stream);
}

extern "C" int lfgc_codec_rans_encode_write(const uint8_t* sym, int64_t n, int rounds, const uint16_t* freq, uint8_t* out,
                                            int64_t out_bytes, void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!sym || !freq || !out || !workspace) return LFGC_E_NULL;
    if (!rans_shape_ok(n, rounds)) return LFGC_E_SHAPE;
    if (((uintptr_t)workspace & 7) || ((uintptr_t)freq & 1) || ((uintptr_t)out & 1)) return LFGC_E_ALIGN;
    RansWorkspace w;
    if (workspace_bytes < rans_workspace(n, rounds, workspace, &w)) return LFGC_E_WORKSPACE;
    if (out_bytes < 2 * kRansHeaderU16 + 260 * w.nc) return LFGC_E_WORKSPACE;
    hipLaunchKernelGGL(rans_encode_kernel<true>, dim3(rans_grid(w.nc)), dim3(kRansBlock), 0, (hipStream_t)stream, sym, (long long)n,
                       rounds, w.nc, freq, w.counts, (const long long*)w.offsets, reinterpret_cast<unsigned short*>(out),
                       (long long)(out_bytes / 2));
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_codec_rans_decode(const uint8_t* in, int64_t in_bytes, int64_t n, int rounds, uint8_t* out, int32_t* status,
                                      void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!in || !out || !status || !workspace) return LFGC_E_NULL;
    if (!rans_shape_ok(n, rounds)) return LFGC_E_SHAPE;
    if (((uintptr_t)workspace & 7) || ((uintptr_t)in & 3) || ((uintptr_t)status & 3)) return LFGC_E_ALIGN;
    RansWorkspace w;
    if (workspace_bytes < rans_workspace(n, rounds, workspace, &w)) return LFGC_E_WORKSPACE;
    if (in_bytes < 2 * kRansHeaderU16 + 260 * w.nc) return LFGC_E_SHAPE;
    LfgcScanTotals totals = {{nullptr, nullptr}};
    const int rc = lfgc_select_scan(reinterpret_cast<const unsigned*>(in + 2 * kRansHeaderU16), w.offsets, w.nc, 1, totals,
                                    (hipStream_t)stream);
    if (rc != LFGC_OK) return rc;
    hipLaunchKernelGGL(rans_decode_kernel, dim3(rans_grid(w.nc)), dim3(kRansBlock), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned short*>(in), (long long)(in_bytes / 2), (long long)n, rounds, w.nc,
                       (const long long*)w.offsets, out, status);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}
