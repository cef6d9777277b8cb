// lfgc_select.h -- order-preserving selection (stream compaction) in three passes, shared by the checkpoint codec
// (lfgc_codec.hip), the ray lists (lfgc_render.hip) and the mesh extraction (lfgc_mesh.hip):
//   count   flags per workgroup of 2048 elements                                  lfgc_select_count_kernel<Pred>
//   scan    exclusive 64-bit scan of the workgroup counts, one workgroup per array lfgc_select_scan (lfgc_select.hip)
//   write   rank(i) = offset of the workgroup + flagged elements before i in it    lfgc_select_write_kernel<Pred, Sink>
// A predicate is  bool operator()(long long i, long long n, Item& item) const  with a nested type Item: false for i >= n,
// and `item` is what the sink stores for a flagged element.  A sink is
//   void operator()(long long i, long long n, bool flag, long long rank, const Item& item) const
// called once for every element of every chunk (also i >= n).  Element order inside a workgroup's chunk: pass j (0..7) x
// wave w (0..3) x lane.  Integer results: bit-exact by construction, no atomics, one writer per output address.
#pragma once
#include "lfgc_common.h"

constexpr int kSelectBlock = 256;
constexpr int kSelectPasses = 8;                                   // elements per thread
constexpr int kSelectPerBlock = kSelectBlock * kSelectPasses;      // elements per workgroup in the count and write passes
constexpr int kSelectMaxArrays = 2;                                // arrays of workgroup counts one scan launch takes

// Workspace of one selection over n elements: offsets[nblocks + 1] (64-bit) | counts[nblocks]; offsets[nblocks] takes the
// total when the caller has no place for it.
struct LfgcSelectWorkspace {
    long long nblocks;
    long long* offsets;
    unsigned* counts;
};

inline long long lfgc_select_blocks(long long n) { return (n + kSelectPerBlock - 1) / kSelectPerBlock; }

// bytes of that workspace (16 for n < 1); with `base`, its carve into *w
inline long long lfgc_select_workspace(long long n, void* base = nullptr, LfgcSelectWorkspace* w = nullptr) {
    if (n < 1) return 16;
    const long long nblocks = lfgc_select_blocks(n);
    if (w) {
        w->nblocks = nblocks;
        w->offsets = reinterpret_cast<long long*>(base);
        w->counts = reinterpret_cast<unsigned*>(w->offsets + nblocks + 1);
    }
    return (nblocks + 1) * 8 + nblocks * 4 + 16;
}

// Where the total of array a goes; null: nowhere.
struct LfgcScanTotals { long long* at[kSelectMaxArrays]; };

// offsets[a * nblocks + b] = counts[a * nblocks] + ... + counts[a * nblocks + b - 1] for a < narrays; *totals.at[a] = the sum
// of array a.  LFGC_OK or the launch error.
int lfgc_select_scan(const unsigned* counts, long long* offsets, long long nblocks, int narrays, LfgcScanTotals totals,
                     hipStream_t stream);

// Sums of N per-thread counts over a 256-thread workgroup: c[k] of thread 0 becomes the workgroup's sum (the other
// threads keep partial sums).  Holds a barrier: every thread of the workgroup calls it.
template <int N>
__device__ __forceinline__ void lfgc_select_block_sum(unsigned (&c)[N]) {
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) c[k] += __shfl_down(c[k], off);
    }
    __shared__ unsigned sw[N][kSelectBlock / 64];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) sw[k][threadIdx.x >> 6] = c[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) c[k] = sw[k][0] + sw[k][1] + sw[k][2] + sw[k][3];
    }
}

namespace {

template <class Pred>
__global__ __launch_bounds__(kSelectBlock) void lfgc_select_count_kernel(const Pred pred, long long n,
                                                                         unsigned* __restrict__ block_counts) {
    const long long base = (long long)blockIdx.x * kSelectPerBlock;
    unsigned c[1] = {0};
    typename Pred::Item item;
#pragma unroll
    for (int j = 0; j < kSelectPasses; ++j) c[0] += pred(base + j * kSelectBlock + threadIdx.x, n, item);
    lfgc_select_block_sum(c);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = c[0];
}

template <class Pred, class Sink>
__global__ __launch_bounds__(kSelectBlock) void lfgc_select_write_kernel(const Pred pred, const Sink sink, long long n,
                                                                         const long long* __restrict__ offsets) {
    const long long base = (long long)blockIdx.x * kSelectPerBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ unsigned s_cnt[kSelectPasses][kSelectBlock / 64];
    bool flag[kSelectPasses];
    typename Pred::Item item[kSelectPasses];
    unsigned long long bal[kSelectPasses];
#pragma unroll
    for (int j = 0; j < kSelectPasses; ++j) {
        flag[j] = pred(base + j * kSelectBlock + threadIdx.x, n, item[j]);
        bal[j] = __ballot(flag[j]);
        if (lane == 0) s_cnt[j][wave] = (unsigned)__popcll(bal[j]);
    }
    __syncthreads();
    long long run = offsets[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kSelectPasses; ++j) {
#pragma unroll
        for (int w = 0; w < kSelectBlock / 64; ++w) {
            if (w == wave)
                sink(base + j * kSelectBlock + threadIdx.x, n, flag[j], run + __popcll(bal[j] & ((1ull << lane) - 1ull)), item[j]);
            run += s_cnt[j][w];
        }
    }
}

// The three passes over n >= 1 elements; the number of flagged elements goes to *count (device), or stays in the workspace
// when count is null.  LFGC_E_WORKSPACE, LFGC_E_UNSUPPORTED (more than 2^31 - 1 workgroups), or the launch error.
template <class Pred, class Sink>
int lfgc_select(const Pred& pred, const Sink& sink, long long n, long long* count, void* workspace, long long workspace_bytes,
                hipStream_t stream) {
    LfgcSelectWorkspace w;
    if (workspace_bytes < lfgc_select_workspace(n, workspace, &w)) return LFGC_E_WORKSPACE;
    if (w.nblocks > 0x7fffffffLL) return LFGC_E_UNSUPPORTED;
    hipLaunchKernelGGL(lfgc_select_count_kernel<Pred>, dim3((unsigned)w.nblocks), dim3(kSelectBlock), 0, stream, pred, n, w.counts);
    LFGC_HIP_CHECK_LAUNCH();
    LfgcScanTotals totals = {{count ? count : w.offsets + w.nblocks, nullptr}};
    const int rc = lfgc_select_scan(w.counts, w.offsets, w.nblocks, 1, totals, stream);
    if (rc != LFGC_OK) return rc;
    hipLaunchKernelGGL((lfgc_select_write_kernel<Pred, Sink>), dim3((unsigned)w.nblocks), dim3(kSelectBlock), 0, stream, pred, sink, n,
                       w.offsets);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

}  // namespace
