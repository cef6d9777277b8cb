// lfgc_f16split.h -- an fp32 operand as an f16 pair x = hi + lo (hi = rne_f16(x), lo = rne_f16(x - hi)): the vector types
// and the conversions the f16-split forward (lfgc_forward16.h) and the backward chains (lfgc_bwd_data.h,
// lfgc_bwd_weight.h) feed v_mfma_f32_32x32x16_f16 with.
#pragma once
#include <utility>
#include "lfgc_common.h"

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <class F, int... I>
__device__ __forceinline__ void lfgc_static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
// f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>): a loop whose index is a constant expression
template <int N, class F>
__device__ __forceinline__ void lfgc_static_for(F&& f) {
    lfgc_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// hi = rne_f16 of a pair (one v_cvt_pk_f16_f32)
__device__ __forceinline__ unsigned lfgc_cvt_pk(float x0, float x1) {
    f32x2 v = {x0, x1};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, h16x2));
}
// lo = rne_f16(x - f32(hi)) of a pair: ONE mixed-precision FMA per value that reads the f16 half in place and writes
// its f16 result into the destination half (hi * -1 + x is exact in fp32, so the only rounding is the final one)
__device__ __forceinline__ unsigned lfgc_lo_pk(unsigned h, float x0, float x1) {
    unsigned l;        // one statement: between two asm statements hipcc puts an s_nop (an issue slot per pair)
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=&v"(l) : "v"(h), "v"(x0), "v"(x1));
    return l;
}

// x[0..8) fp32 -> hi / lo f16 fragments, 1.5 VALU instructions per value.
__device__ __forceinline__ void lfgc_split8(const float* __restrict__ x, h16x8& hi, h16x8& lo) {
    u32x4 hp, lp;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        hp[t] = lfgc_cvt_pk(x[2 * t], x[2 * t + 1]);
        lp[t] = lfgc_lo_pk(hp[t], x[2 * t], x[2 * t + 1]);
    }
    hi = __builtin_bit_cast(h16x8, hp);
    lo = __builtin_bit_cast(h16x8, lp);
}

// Reduced-precision build (LFGC_PRECISION_F16): the hi half only, one packed conversion per pair.
__device__ __forceinline__ void lfgc_cvt8(const float* __restrict__ x, h16x8& hi) {
    u32x4 hp;
#pragma unroll
    for (int t = 0; t < 4; ++t) hp[t] = lfgc_cvt_pk(x[2 * t], x[2 * t + 1]);
    hi = __builtin_bit_cast(h16x8, hp);
}
