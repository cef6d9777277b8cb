// lfgc_select.hip -- the scan pass of the order-preserving selection (lfgc_select.h): the one kernel of it that is no
// template, compiled here once for the codec, the ray lists and the mesh.
#include "lfgc_select.h"

namespace {

// Workgroup a (1024 threads = 16 waves) scans array a in rounds of 1024 counts: wave-inclusive scan by shuffles, the 16
// wave totals through LDS, the sum of the earlier rounds carried in s_carry.
__global__ __launch_bounds__(1024) void select_scan_kernel(const unsigned* __restrict__ counts, long long* __restrict__ offsets,
                                                           long long nblocks, const LfgcScanTotals totals) {
    counts += blockIdx.x * nblocks;
    offsets += blockIdx.x * nblocks;
    __shared__ long long s_wave[16];
    __shared__ long long s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (long long b0 = 0; b0 < nblocks; b0 += 1024) {
        const long long b = b0 + threadIdx.x;
        const long long v = b < nblocks ? counts[b] : 0;
        long long incl = v;
        for (int off = 1; off < 64; off <<= 1) {
            const long long t = __shfl_up(incl, off);
            if ((threadIdx.x & 63) >= off) incl += t;
        }
        if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
        __syncthreads();
        long long wave_off = 0;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) wave_off += s_wave[w];
        const long long carry = s_carry;
        if (b < nblocks) offsets[b] = carry + wave_off + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) s_carry = carry + wave_off + incl;
        __syncthreads();
    }
    long long* total = blockIdx.x == 0 ? totals.at[0] : totals.at[1];
    if (threadIdx.x == 0 && total) *total = s_carry;
}

}  // namespace

int lfgc_select_scan(const unsigned* counts, long long* offsets, long long nblocks, int narrays, LfgcScanTotals totals,
                     hipStream_t stream) {
    static_assert(kSelectMaxArrays == 2, "select_scan_kernel picks the total's place between two");
    if (narrays < 1 || narrays > kSelectMaxArrays) return LFGC_E_SHAPE;
    hipLaunchKernelGGL(select_scan_kernel, dim3((unsigned)narrays), dim3(1024), 0, stream, counts, offsets, nblocks, totals);
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}
