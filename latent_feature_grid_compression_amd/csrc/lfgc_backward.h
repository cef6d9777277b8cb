// lfgc_backward.h -- backward of the fused sample + embed + MLP path for gfx950 (exact fp32 MFMA).
//
// What autograd derives for model/Feature_Grid_Model.py:62-75 in the reference (triggered at
// training/training.py:137), as three kernels:
//   1. lfgc_bwd_data_kernel   per 32-sample wave tile, the forward's register mapping run backwards:
//        dH_L = Wf dy ; for l = L..1: dA_l = dH_l * snake'(a_l) (a_l from the forward's stash),
//        dH_{l-1} = W_l^T dA_l  (A operand = transposed weight image in LDS, B operand = dA_l in VGPRs,
//        the accumulators are again the next step's B operand), dX0 = W_0^T dA_1 lands in exactly the
//        registers the forward's layer-0 input occupied: grid-feature gradients -> float-atomic scatter into
//        the channel-last d_grid (staged through LDS so that one atomic wave-instruction covers whole 128-B
//        channel rows), scalar-input gradients (+ the sampler's coordinate gradient) -> d_pos.
//        dA_l is also written to a scratch "dstash" for kernel 2.
//   2. lfgc_bwd_weight_kernel  dW_l = dA_l^T H_{l-1}: contraction over SAMPLES (K = 32 per tile), M = h_out,
//        N = k_in; operands are read back from stash/dstash so that 16 consecutive samples of one row are one
//        64-byte load per lane; each workgroup accumulates its share of the sample tiles in registers and
//        writes one partial slab.
//   3. lfgc_bwd_reduce_kernel  sums the slabs into the nn.Linear-shaped gradients (deterministic, no atomics).
//
// This header is what the host entry (lfgc_backward.hip) needs: the argument structs and the LDS, slab and fixed-point
// layouts.  The kernels are templates in lfgc_bwd_data.h (1, with the feature-gradient scatters; all the input-gradient
// build includes) and lfgc_bwd_weight.h (2); the kernels that are no templates (3 and the fixed-point scatter's passes)
// are compiled once, in lfgc_backward.hip.
#pragma once
#include "lfgc_common.h"

struct LfgcBwdArgs {
    const float* pos;          // (N,3)
    long long n;
    const float* grid;         // (D,H,W,Cs)   (read only when d_pos is requested)
    int D, H, W, Cs;
    const float* packed;
    int L;
    const float* stash;
    const float* d_out;        // (N) (the INPUT_ONLY build: or nullptr = ones)
    float* dstash;             // [tiles][L*16*MT][64]
    float* dscale;             // [tiles][L]: the power-of-two scale each tile's dA_l was split with (f16 builds), for the weight kernel
    float* d_grid;             // (D,H,W,Cs), accumulated with float atomics
    float* dfeat;              // nullptr: the data kernel scatters into d_grid itself; else (tiles*32, CH) scratch: it only
                               // writes the feature gradients there and lfgc_bwd_scatter_kernel does the atomics
    float* d_pos;              // (N,3) or nullptr (the INPUT_ONLY build: never nullptr)
    long long nbatches;
    unsigned long long* stamps;   // diagnostics builds (-DLFGC_STAMPS, tools/phase_stamps.py bwd): per-wave cycle totals per phase
};

// Dynamic LDS of lfgc_bwd_data_kernel in floats, in the order the kernel carves it:
//   s_final [Wf (HP) | bf (4)] | s_inv 8 | s_ring: 2 slots, each a transposed weight image (tblk0 / tblk1) or, once the
//   layer-0 image is consumed, the scatter staging of all `waves` waves (scatter_wave() each).
// The host's launch selection sizes the allocation with lfgc_bwd_lds_floats; the kernel takes its slot from the same function.
constexpr int lfgc_bwd_lds_slot(const LfgcPlan& p, int waves) {
    const int img = p.tblk0 > p.tblk1 ? p.tblk0 : p.tblk1, sc = waves * p.scatter_wave();
    return img > sc ? img : sc;
}
constexpr int lfgc_bwd_lds_floats(const LfgcPlan& p, int waves) { return p.HP + 4 + 8 + 2 * lfgc_bwd_lds_slot(p, waves); }

// ---------------------------------------------------------------------------------------------------------
// order-independent scatter (lfgc_backward_det_f32): 64-bit fixed point, integer atomics
// ---------------------------------------------------------------------------------------------------------
// d_grid[i] = q * sum round(v w / q) with ONE power-of-two quantum q per call: integer addition is associative, so the
// sum depends on neither the order of the samples nor the launch geometry.  Steps, all on the call's stream:
//   lfgc_det_zero_kernel     acc = 0, max word = 0 (a kernel, not a memset node: DESIGN.md 3.1)
//   lfgc_det_max_kernel      max word = max bits of |dfeat| over the n valid rows (unsigned atomicMax: order-independent;
//                            a non-finite value is any bits >= 0x7f800000 and wins the maximum)
//   lfgc_bwd_scatter_det_kernel   lfgc_bwd_scatter_kernel's walk (lfgc_scatter_walk); the fp32 product v w is scaled exactly
//                            in double by 1 / q, rounded to nearest and added with a 64-bit integer atomic
//   lfgc_det_finish_kernel   d_grid[i] = (float)(acc[i] q) for EVERY element (zeros included: d_grid needs no zero fill);
//                            max == 0: all zero; non-finite max: all NaN
struct LfgcDetScatter {
    long long* acc;            // (D,H,W,Cs) int64 fixed-point accumulator (workspace)
    unsigned* maxw;            // max bits of |dfeat| (workspace)
};

constexpr unsigned kLfgcDetNonFinite = 0x7f800000u;

// Exponent of the quantum, q = 2^(E - B): 2^E >= max (E minimal) and B = 61 - ceil(log2(8 n)).  Corner weights are <= 1
// and at most 8 n contributions meet at one address, so |sum| <= 8 n 2^B <= 2^61: a quarter of the int64 range.
// max_bits = 0, non-finite bits or n < 1 have no quantum: 0.
__host__ __device__ inline int lfgc_det_qexp(unsigned max_bits, long long n) {
    if (max_bits == 0u || max_bits >= kLfgcDetNonFinite || n < 1) return 0;
    const int e = (int)(max_bits >> 23);
    const unsigned mant = max_bits & 0x7fffffu;
    int E;
    if (e == 0) E = (mant == 1u ? 0 : 32 - __builtin_clz(mant - 1u)) - 149;        // subnormal: mant 2^-149
    else E = e - 127 + (mant != 0u);
    const unsigned long long m = 8ull * (unsigned long long)n;                     // >= 8
    const int B = 61 - (64 - __builtin_clzll(m - 1ull));
    return E - B;
}

// 2^k as a double for |k| <= 1022 (lfgc_det_qexp is within [-207, 102])
__device__ __forceinline__ double lfgc_det_pow2(int k) {
    return __longlong_as_double((long long)(1023 + k) << 52);
}

// lfgc_det_max_kernel over `count` floats of dfeat, on `stream` (lfgc_backward.hip; the per-channel launchers of
// lfgc_bwd_weight.h put it in front of their lfgc_bwd_scatter_det_kernel).
int lfgc_launch_det_max(const float* dfeat, long long count, unsigned* maxw, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------
// weight gradients
// ---------------------------------------------------------------------------------------------------------
struct LfgcWgradArgs {
    const float* stash;
    const float* dstash;
    const float* d_out;
    long long n;
    long long ntiles;          // 32-sample tiles that hold data (multiple of 4: whole workgroup batches)
    int L;
    float* slabs;              // [gridDim.x / roles][slab_floats]
    int slab_floats;
    int roles;                 // 1: a workgroup computes every layer's gradient for its tiles (one slab per workgroup);
                               // L: workgroup b computes layer b % L only (the last role also the head) for the tiles of
                               // group b / L -- a quarter of the slabs for the same operand reads
    const float* dscale;       // [tiles][L] from the data kernel, or nullptr: exact f32 MFMA contraction
};

// Slab layout (floats): per hidden layer l: dW [HP][NC_l] (NC_0 = K0R in packed column order, else HP) | db [HP];
// then final layer: dWf [HP] | dbf [4].
__host__ __device__ constexpr int lfgc_slab_layer_off(const LfgcPlan& p, int l) {
    return l == 0 ? 0 : p.slab_blk0() + (l - 1) * p.slab_blk1();
}
__host__ __device__ constexpr int lfgc_slab_floats(const LfgcPlan& p) { return lfgc_slab_layer_off(p, p.L) + p.HP + 4; }
