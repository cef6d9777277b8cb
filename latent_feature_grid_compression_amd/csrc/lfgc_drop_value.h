// lfgc_drop_value.h -- the pruning layers' value rule, shared by every kernel that folds a drop layer into a wavelet
// level (lfgc_wavelet.hip: channel-first levels, lfgc_wavelet_cl.hip: the channel-last last level).
#pragma once
#include <hip/hip_runtime.h>

// One coefficient through its drop layer (model/Smallify_Dropout.py:57, model/Variational_Dropout_Layer.py:109,
// model/Straight_Through_Dropout.py:28 and :58 -- the latter op for op, so the value is the reference's bit for bit).
__device__ __forceinline__ float drop_value(float x, float m, float thr, bool ste) {
    if (!ste) return __fmul_rn(x, m);
    const float hard = m >= thr ? 1.0f : 0.0f;
    const float soft = __fmul_rn(x, m);
    return __fadd_rn(__fsub_rn(__fmul_rn(x, hard), soft), soft);
}

__device__ __forceinline__ float sign_of(float v) { return (float)((v > 0.0f) - (v < 0.0f)); }
