/* lfgc.h -- C-ABI of liblfgc.so: the MI355X (gfx950) implementation of the latent-feature-grid
 * sample/decode hot path of Bussler/Latent_Feature_Grid_Compression.
 *
 * The reference has no FFI: its "interface" for this path is the Python nn.Module
 * model/Feature_Grid_Model.py (forward :50-80, decode_volume :102-108, encode_volume :83-99), the
 * wavelet filter wavelet_transform/Torch_Wavelet_Transform.py (encode :75-89, decode :91-104) and
 * the ground-truth sampler data/Interpolation.py:8-44.  Each entry point below names the reference
 * lines it replaces.  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer marked "device" is a HIP device pointer owned by the caller (e.g. a torch tensor's
 *     data_ptr()); "host" pointers are ordinary host memory read before the call returns;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream); the
 *     call returns without synchronising; no entry point allocates device memory or synchronises;
 *   - return value: 0 = LFGC_OK, negative = LFGC_E_* argument/shape error (nothing was launched),
 *     positive = the hipError_t of a failed launch.  Never aborts, never throws;
 *   - all floating-point data is IEEE fp32, tensors are dense/contiguous in the stated layout.
 */
#ifndef LFGC_H
#define LFGC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFGC_VERSION 100          /* 0.1.0 */
#define LFGC_MAX_LAYERS 8         /* hidden layers (reference default 4, model/Feature_Grid_Model.py:18) */

enum {
    LFGC_OK = 0,
    LFGC_E_NULL = -1,             /* required pointer is NULL */
    LFGC_E_SHAPE = -2,            /* negative / zero / inconsistent extent */
    LFGC_E_UNSUPPORTED = -3,      /* shape outside the compiled kernel set (see lfgc_mlp_supported) */
    LFGC_E_ALIGN = -4,            /* pointer not 16-byte aligned where required */
    LFGC_E_WORKSPACE = -5         /* workspace / packed buffer too small */
};

typedef void* lfgc_stream_t;      /* hipStream_t */

int lfgc_version(void);
const char* lfgc_error_string(int code);

/* ------------------------------------------------------------------------------------------------
 * Wavelet transform of the feature grid
 * ---------------------------------------------------------------------------------------------- */

/* One inverse-DWT level.  Replaces _WaveletFilterNd.decode + _unpad_for_reverse
 * (wavelet_transform/Torch_Wavelet_Transform.py:91-104, :69-73) as called per level from
 * Feature_Grid_Model.decode_volume (model/Feature_Grid_Model.py:104-107): torch.cat of the LLL band
 * with the 7 detail bands, grouped conv_transpose3d (stride 2, 4^3 taps), crop to `t`.
 *   lll        device (C, d0,d1,d2)           low band (coarse parameter or previous level's output)
 *   hf         device (C, 7, d0,d1,d2)        detail bands, sub-band s = 4a+2b+c stored at hf[:, s-1]
 *   filter_rev device (8, 4,4,4)              the module's `filter.filter_rev` buffer (fp32)
 *   taps       host float[8] or NULL          the 1-D bank [low taps | high taps] (pywt rec_lo, rec_hi cast to fp32) IF
 *                                             filter_rev is its outer product a[sz][tz]*(a[sy][ty]*a[sx][tx]), the only way the
 *                                             reference builds it (Torch_Wavelet_Transform.py:39-57): the stencil is then
 *                                             contracted axis by axis (224 instead of 512 FMAs per 8 outputs; results equal
 *                                             the dense form up to fp32 rounding) and filter_rev may be NULL
 *   out        device (C, t0,t1,t2)
 * Requires 2*d_a + 2 >= t_a >= 1 (4 taps; the *_len_f32 entries below take other lengths).  The same `taps` convention applies to every wavelet entry point below. */
int lfgc_idwt_level_f32(const float* lll, const float* hf, const float* filter_rev, const float* taps, float* out,
                        int C, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream);

/* Adjoint of lfgc_idwt_level_f32 (what autograd derives for the ops above; triggered at
 * training/training.py:137): d_lll (C,d0,d1,d2) and d_hf (C,7,d0,d1,d2) are OVERWRITTEN with the
 * gradients given d_out (C, t0,t1,t2). */
int lfgc_idwt_level_bwd_f32(const float* d_out, const float* filter_rev, const float* taps, float* d_lll, float* d_hf,
                            int C, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream);

/* Layout conversion of a dense grid between the reference's channel-first (C, V) = decode_volume()'s output
 * (model/Feature_Grid_Model.py:108) and the channel-last (V, channel_stride) form the sampler and the gradient
 * scatter use (V = D*H*W voxels, channel_stride = lfgc_grid_channel_stride(C), pad channels written as 0).
 * to_channel_last != 0: src (C,V) -> dst (V,cs); else src (V,cs) -> dst (C,V).  src != dst. */
int lfgc_grid_layout_f32(const float* src, float* dst, int C, int64_t voxels, int channel_stride,
                         int to_channel_last, lfgc_stream_t stream);

/* The LAST level of decode_volume() written straight in the sampler's channel-last layout, and its adjoint reading the
 * gradient of that layout: lfgc_idwt_level_f32 + lfgc_grid_layout_f32 (and lfgc_grid_layout_f32 +
 * lfgc_idwt_level_bwd_f32) in one pass over the data each (wavelet_transform/Torch_Wavelet_Transform.py:91-104, crop
 * :69-73; the permute is this library's, the reference samples the channel-first grid).
 *   out_cl / d_out_cl  device (t0,t1,t2, channel_stride), channel_stride = lfgc_grid_channel_stride(C); pad channels
 *                      are written as 0 / ignored
 *   taps               REQUIRED (separable bank, see above).  Returns LFGC_E_UNSUPPORTED for taps == NULL or arrays of
 *                      2^30 bytes and more: the caller then composes the two channel-first entry points.
 *   C                  any C >= 1: channel groups of 32, 16 or 8 (lfgc_idwt_level_cl_plan below) cover every stride
 *                      that is a multiple of 8.  C > 32 is taken by this plain pair only (tests/test_wavelet_cl_paths_gpu.py
 *                      runs C = 40 and 48); the drop pair below refuses it, and nobody has timed such a level against the
 *                      two-kernel form. */
int lfgc_idwt_level_cl_f32(const float* lll, const float* hf, const float* taps, float* out_cl,
                           int C, int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream);
int lfgc_idwt_level_cl_bwd_f32(const float* d_out_cl, const float* taps, float* d_lll, float* d_hf,
                               int C, int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream);

/* One forward-DWT level (init only).  Replaces _WaveletFilterNd.encode incl. _pad_for_forward
 * (wavelet_transform/Torch_Wavelet_Transform.py:59-67, :75-89): zero-pad (2, 2 + odd) per axis,
 * grouped conv3d stride 2.  in (C, n0,n1,n2) -> out (C, 8, d0,d1,d2), d_a = (n_a + pad_hi_a) / 2 + 1 - ...
 * exactly: d_a = (n_a + 2 + 2 + odd_a' - 4) / 2 + 1 where odd_a' is the reference's pad-slot quirk
 * (the odd bit of axis a lands on axis 2-a).  filter_fwd device (8,4,4,4); taps = its 1-D bank (pywt dec_lo, dec_hi,
 * each flipped) or NULL. */
int lfgc_dwt_level_f32(const float* in, const float* filter_fwd, const float* taps, float* out,
                       int C, int n0, int n1, int n2, lfgc_stream_t stream);

/* The same seven entry points for any even filter length L = filter_len in {2, 4, 6, 8} (Haar / db1, db2, db3, db4 and
 * any other even-length bank: the reference's filter module takes any pywt wavelet, Torch_Wavelet_Transform.py:11-14,
 * :32-33; its options expose it as --wavelet_filter, Feature_Grid_Training.py:62).  The arithmetic is the reference's
 * conv_transpose3d / conv3d for an L^3 filter: one level's full output is 2 d_a + L - 2 per axis, so
 *   1 <= t_a <= 2 d_a + L - 2,  crop offset floor((2 d_a + L - 2 - t_a) / 2)  (_unpad_for_reverse, :69-73),
 * and the forward DWT pads (2L - 3) // 2 = L - 2 per side plus the odd bit on the high side, with the same pad-slot quirk
 * (_get_padding_size, :59-63): d_a = (n_a + 2 (L - 2) + odd_a' - L) / 2 + 1.
 *   filter_rev / filter_fwd  device (8, L,L,L) -- only read for L = 4 with taps == NULL (dense stencil)
 *   taps                     host float[2 * L] [low taps | high taps], REQUIRED for L != 4 (the reference only ever
 *                            builds outer products, :39-57); a dense filter of another length returns LFGC_E_UNSUPPORTED
 * Other lengths return LFGC_E_UNSUPPORTED.  filter_len = 4 is exactly the plain entry point above.  The channel-last pair
 * takes L = 2 and 4 and returns LFGC_E_UNSUPPORTED for L = 6, 8 (compose the channel-first level with
 * lfgc_grid_layout_f32).  The drop pair is declared with the drop entry points below.
 * Width limit: a workgroup of the channel-first synthesis stages whole coefficient rows in LDS (at most 160 KB), so the
 * LAST coefficient extent d2 is bounded per filter length -- every d2 up to
 *   L = 2: 853    L = 4: 373    L = 6: 169    L = 8: 96
 * is taken (for any d0, d1, t); past it the synthesis and its drop variant return LFGC_E_UNSUPPORTED before anything is
 * launched.  The adjoint takes every level the synthesis takes (at the full t its own limit is d2 = 1280, 560, 318, 201).
 * The forward DWT stages source rows and takes every LAST source extent n2 up to
 *   L = 2: 2560   L = 4: 1122   L = 6: 638    L = 8: 408
 * which covers the output 2 d2 + L - 2 of every level inside the synthesis limit.  The lfgc_*_plan queries below answer
 * for a given shape (tests/test_wavelet_plans_host.py pins these tables). */
int lfgc_idwt_level_len_f32(const float* lll, const float* hf, const float* filter_rev, const float* taps, int filter_len,
                            float* out, int C, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream);
int lfgc_idwt_level_bwd_len_f32(const float* d_out, const float* filter_rev, const float* taps, int filter_len,
                                float* d_lll, float* d_hf, int C, int d0, int d1, int d2, int t0, int t1, int t2,
                                lfgc_stream_t stream);
int lfgc_idwt_level_cl_len_f32(const float* lll, const float* hf, const float* taps, int filter_len, float* out_cl,
                               int C, int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream);
int lfgc_idwt_level_cl_bwd_len_f32(const float* d_out_cl, const float* taps, int filter_len, float* d_lll, float* d_hf,
                                   int C, int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2,
                                   lfgc_stream_t stream);
int lfgc_dwt_level_len_f32(const float* in, const float* filter_fwd, const float* taps, int filter_len, float* out,
                           int C, int n0, int n1, int n2, lfgc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Pruning ("drop") layers on the wavelet coefficients
 *
 * Every drop layer of the reference multiplies a coefficient tensor (C, ...) by a per-coefficient factor m of
 * shape (...) that is shared by all channels (`x.mul(self.betas.unsqueeze(0))` and relatives):
 *   SmallifyDropout.forward                        model/Smallify_Dropout.py:54-61         m = betas | d_mask
 *   Straight_Through_Dropout.forward               model/Straight_Through_Dropout.py:26-30  m = (rand < mask_values)
 *   MaskedWavelet_Straight_Through_Dropout.forward model/Straight_Through_Dropout.py:54-62  m = sigmoid(mask_values), thr
 *   VariationalDropout.forward                     model/Variational_Dropout_Layer.py:101-112  m = theta + sigma*xi | d_mask
 * `threshold` selects the value rule: NaN -> value = x*m; otherwise the masked straight-through rule
 * value = (x*(m >= threshold) - x*m) + x*m (forward value of the hard mask, gradient of the soft one).
 * In both rules the gradients are d_x = g*m and d_m = sum over channels of g*x.
 * ---------------------------------------------------------------------------------------------- */

/* lfgc_idwt_level_f32 with the drop layers of its inputs folded in (model/Feature_Grid_Model.py:103, :105):
 *   mul_lll device (d0,d1,d2) or NULL     factor of the low band (only the coarsest level has one: drop[0])
 *   mul_hf  device (7, d0,d1,d2) or NULL  factor of the detail bands (drop[level]) */
int lfgc_idwt_level_drop_f32(const float* lll, const float* hf, const float* mul_lll, float threshold_lll,
                             const float* mul_hf, float threshold_hf, const float* filter_rev, const float* taps, float* out,
                             int C, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream);

/* Adjoint of lfgc_idwt_level_drop_f32: d_lll / d_hf are OVERWRITTEN with the gradients of the UN-multiplied inputs;
 * the factor gradients are ADDED (float atomics over the channels) into d_mul_lll (d0,d1,d2) / d_mul_hf (7,d0,d1,d2),
 * which the caller zero-fills beforehand (NULL = not wanted; wanting them needs lll / hf).
 * penalty_grads: NULL, or a HOST array of 4 device pointers to single floats (each may be NULL) = the upstream gradients
 * of penalty terms whose own gradients are folded into this pass instead of costing a pass of their own:
 *   [0] d(loss)/d(sum lll^2)   -> d_lll += 2 g lll        (only where lll is a parameter: the coarsest level)
 *   [1] d(loss)/d(sum hf^2)    -> d_hf  += 2 g hf         (ΣG² term of SmallifyLoss / VariationalDropoutLoss)
 *   [2] d(loss)/d(sum |mul_lll|), [3] d(loss)/d(sum |mul_hf|) -> d_mul += g sign(mul), for a factor that is itself the
 *       penalised parameter (SmallifyDropout.betas, model/Smallify_Dropout.py:63-64). */
int lfgc_idwt_level_drop_bwd_f32(const float* d_out, const float* filter_rev, const float* taps, const float* lll, const float* hf,
                                 const float* mul_lll, const float* mul_hf, float* d_lll, float* d_hf,
                                 float* d_mul_lll, float* d_mul_hf, const float* const* penalty_grads,
                                 int C, int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream);

/* lfgc_idwt_level_drop_f32 / lfgc_idwt_level_drop_bwd_f32 for filter length filter_len (see lfgc_idwt_level_len_f32). */
int lfgc_idwt_level_drop_len_f32(const float* lll, const float* hf, const float* mul_lll, float threshold_lll,
                                 const float* mul_hf, float threshold_hf, const float* filter_rev, const float* taps,
                                 int filter_len, float* out, int C, int d0, int d1, int d2, int t0, int t1, int t2,
                                 lfgc_stream_t stream);
int lfgc_idwt_level_drop_bwd_len_f32(const float* d_out, const float* filter_rev, const float* taps, int filter_len,
                                     const float* lll, const float* hf, const float* mul_lll, const float* mul_hf,
                                     float* d_lll, float* d_hf, float* d_mul_lll, float* d_mul_hf,
                                     const float* const* penalty_grads, int C, int d0, int d1, int d2,
                                     int t0, int t1, int t2, lfgc_stream_t stream);

/* The LAST level with drop layers, in the sampler's channel-last layout: lfgc_idwt_level_drop_len_f32 + lfgc_grid_layout_f32
 * (and lfgc_grid_layout_f32 + lfgc_idwt_level_drop_bwd_len_f32) in one pass over the data each.  Thresholds, overwritten
 * and accumulated outputs, pre-zeroed d_mul_* and penalty_grads[4] are those of the channel-first drop pair above, word for
 * word; layouts, pad channels, crop and limits are those of the channel-last pair (out_cl / d_out_cl (t0,t1,t2,
 * channel_stride), channel_stride = lfgc_grid_channel_stride(C), separable bank `taps` REQUIRED).  filter_len is 2 or 4.
 * Decided before anything is launched: LFGC_E_NULL for a missing required pointer (lll / hf included where a d_mul_* or an
 * L2 penalty needs them); LFGC_E_SHAPE for channel_stride != C rounded up to 8 or t_a out of range; LFGC_E_UNSUPPORTED for
 * taps == NULL, another filter_len, C > 32 or an array of 2^30 bytes and more (compose the channel-first drop entry with
 * the layout conversion).  With all four factor and penalty pointers NULL they are exactly the plain channel-last pair. */
int lfgc_idwt_level_cl_drop_len_f32(const float* lll, const float* hf, const float* mul_lll, float threshold_lll,
                                    const float* mul_hf, float threshold_hf, const float* taps, int filter_len,
                                    float* out_cl, int C, int channel_stride, int d0, int d1, int d2,
                                    int t0, int t1, int t2, lfgc_stream_t stream);
int lfgc_idwt_level_cl_drop_bwd_len_f32(const float* d_out_cl, const float* taps, int filter_len,
                                        const float* lll, const float* hf, const float* mul_lll, const float* mul_hf,
                                        float* d_lll, float* d_hf, float* d_mul_lll, float* d_mul_hf,
                                        const float* const* penalty_grads, int C, int channel_stride,
                                        int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream);

/* The two drop adjoints with bitwise repeatable factor gradients: every address of a factor-gradient array gets exactly
 * ONE add.  slice_stride (floats) > 0: d_mul_lll / d_mul_hf are ZERO-FILLED scratch of S slices, slice s at d_mul_* + s *
 * slice_stride; the channel-first entry writes channel c into slice c (S = C), the channel-last entry writes its channel
 * group into one slice each (S = channel_stride / 16 where that divides, else channel_stride / 8).  The L1 penalty term
 * goes to slice 0.  lfgc_sum_slices_f32 then folds the slices in the order 0 .. S-1 into the factor gradient.
 * slice_stride must hold the larger factor wanted (7 d0 d1 d2 with d_mul_hf, else d0 d1 d2), else LFGC_E_SHAPE.
 * slice_stride == 0 IS the plain entry (float atomics over the channels); every other argument, check and return code
 * is the plain entry's. */
int lfgc_idwt_level_drop_bwd_det_len_f32(const float* d_out, const float* filter_rev, const float* taps, int filter_len,
                                         const float* lll, const float* hf, const float* mul_lll, const float* mul_hf,
                                         float* d_lll, float* d_hf, float* d_mul_lll, float* d_mul_hf,
                                         int64_t slice_stride, const float* const* penalty_grads, int C,
                                         int d0, int d1, int d2, int t0, int t1, int t2, lfgc_stream_t stream);
int lfgc_idwt_level_cl_drop_bwd_det_len_f32(const float* d_out_cl, const float* taps, int filter_len,
                                            const float* lll, const float* hf, const float* mul_lll, const float* mul_hf,
                                            float* d_lll, float* d_hf, float* d_mul_lll, float* d_mul_hf,
                                            int64_t slice_stride, const float* const* penalty_grads, int C,
                                            int channel_stride, int d0, int d1, int d2, int t0, int t1, int t2,
                                            lfgc_stream_t stream);
/* out[i] = ((slices[i] + slices[stride + i]) + slices[2 stride + i]) + ... over nslices slices, i < n <= stride: fixed
 * order, no atomics.  out may be slice 0 itself. */
int lfgc_sum_slices_f32(const float* slices, int nslices, int64_t stride, int64_t n, float* out, lfgc_stream_t stream);

/* One drop layer on one tensor outside the decode (the layers' own forward(x)): x, out (C, n), mul (n). */
int lfgc_drop_apply_f32(const float* x, const float* mul, float threshold, float* out, int C, int64_t n,
                        lfgc_stream_t stream);
int lfgc_drop_apply_bwd_f32(const float* d_out, const float* x, const float* mul, float* d_x, float* d_mul /* or NULL */,
                            int C, int64_t n, lfgc_stream_t stream);

/* SmallifySignVarianceTracker.sign_variance_pruning_onlyVar (model/Smallify_Dropout.py:106-112) on DEVICE state:
 * phi = sign(betas) - ema; ema += momentum*phi; emavar = (1 - momentum)*(emavar + momentum*phi^2), fp32, the
 * reference's operation order (bit-identical state; the reference moves betas to the CPU every step).  sign is
 * torch.sign's (b > 0) - (b < 0): +0 for -0 and for a NaN beta of either sign, so a NaN beta reads as 0. */
int lfgc_sign_variance_update_f32(const float* betas, float* ema, float* emavar, float momentum, int64_t n,
                                  lfgc_stream_t stream);
/* The same step for all drop layers of a model in one launch: host arrays of n_layers (<= LFGC_PENALTY_MAX_TERMS)
 * device pointers and lengths. */
int lfgc_sign_variance_update_multi_f32(const float* const* betas, float* const* ema, float* const* emavar,
                                        const int64_t* n, int n_layers, float momentum, lfgc_stream_t stream);

/* Penalty terms of the pruning losses as ONE multi-tensor reduction (SmallifyLoss, model/Smallify_Dropout.py:21-40;
 * VariationalDropoutLoss._collect_penalties + calculate_Dkl, model/Variational_Dropout_Layer.py:48-53, :115-122). */
enum {
    LFGC_PENALTY_L1 = 0,          /* sum |a|                 (l1_loss of betas / mask_values)               */
    LFGC_PENALTY_L2 = 1,          /* sum a^2                 (torch.sum(torch.abs(f) ** 2) of a coefficient tensor) */
    LFGC_PENALTY_DKL = 2          /* sum -k1*sigmoid(k2 + k3*la) + 0.5*softplus(-la) + k1, la = b - 2a (a = log_thetas, b = log_var) */
};
#define LFGC_PENALTY_MAX_TERMS 16
typedef struct lfgc_penalty_term {
    const float* a;               /* device */
    const float* b;               /* device, DKL only */
    int64_t n;
    int32_t kind;
} lfgc_penalty_term;
/* terms: host array; sums: device double[LFGC_PENALTY_SUMS_DOUBLES(n_terms)]: the first n_terms entries receive the
 * results (fp64 accumulation, fixed summation order: bitwise repeatable), the rest is scratch (per-workgroup partials). */
#define LFGC_PENALTY_BLOCKS 1024
#define LFGC_PENALTY_SUMS_DOUBLES(n_terms) ((n_terms) * (1 + LFGC_PENALTY_BLOCKS))
int lfgc_penalty_sums_f32(const lfgc_penalty_term* terms, int n_terms, double* sums, lfgc_stream_t stream);
/* Gradients: grad_a[t] (and grad_b[t] for DKL terms) are OVERWRITTEN with d_sums[t] * d(term t)/d(a | b);
 * d_sums device float[n_terms]; grad_a / grad_b host arrays of device pointers. */
int lfgc_penalty_grads_f32(const lfgc_penalty_term* terms, int n_terms, const float* d_sums,
                           float* const* grad_a, float* const* grad_b, lfgc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Binary checkpoint codec, device side.  The reference's store_model_parameters /
 * restore_model (model/model_utils.py:120-332) do the per-coefficient work in Python lists and strings; these entry
 * points are that work on device buffers.  File layout, header and the hidden-layer / final-layer fields are host code
 * (latent_feature_grid_compression_amd/model/model_utils.py); byte order of every packed stream: MSB first.
 * ---------------------------------------------------------------------------------------------- */

/* Bit mask "1 = coefficient != 0" of x[0..n) (model_utils.py:204-208 + binary_writing :89-107): mask has (n+7)/8 bytes,
 * bit i at byte i/8, MSB first, tail bits zero. */
int lfgc_codec_mask_f32(const float* x, int64_t n, uint8_t* mask, lfgc_stream_t stream);

/* Workspace of the two order-preserving passes below. */
int64_t lfgc_codec_select_workspace_bytes(int64_t n);

/* out[0..*count) = the non-zero values of x in order (model_utils.py:210-212: nonzero + index); count: device int64. */
int lfgc_codec_compact_f32(const float* x, int64_t n, float* out, int64_t* count, void* workspace,
                           int64_t workspace_bytes, lfgc_stream_t stream);

/* out[i] = mask bit (bit_offset + i) ? values[rank of that bit among the set bits of [bit_offset, bit_offset + i)] : 0
 * (restore_model's zero re-insertion, model_utils.py:297-306, there one np.insert per pruned element).  The number of set
 * bits of the range, the selection's scanned total, is left in the workspace as the int64 at index ceil(n / 2048), behind
 * the workgroup offsets: a caller that has to verify it reads it there. */
int lfgc_codec_expand_f32(const uint8_t* mask, int64_t bit_offset, int64_t n, const float* values, float* out,
                          void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);

/* k-entry codebook (k <= 256) of the values x[0..n) by `iterations` Lloyd steps from the SORTED initial centres passed in
 * `centres` (overwritten, stays sorted); labels (uint8, optional) = index of the nearest final centre.  Replaces
 * kmeans_quantization (model_utils.py:65-70: scikit-learn KMeans(n_clusters, n_init=4), unseeded -> the reference's own
 * codebooks are not reproducible; any codebook is a valid file).  Deterministic: per-workgroup partial sums folded in a
 * fixed order. */
/* HOST function (no device work): k sorted initial centres from a SORTED host sample of the values (n <= 2^24) by
 * agglomerative merging of adjacent clusters (Ward's criterion) until k remain; n <= k: the values themselves, padded. */
int lfgc_codec_ward_init_host(const float* sorted_values, int64_t n, int k, float* centres);
#define LFGC_CODEC_KMEANS_PARTS 1024
int64_t lfgc_codec_kmeans_workspace_bytes(int k);
int lfgc_codec_kmeans1d_f32(const float* x, int64_t n, int k, float* centres, uint8_t* labels, int iterations,
                            void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);

/* The same codebook construction for k up to 65 536 (label widths 9 to 16), over the values SORTED ascending by the caller.
 * The Lloyd iteration is the one above, step for step: `centres` holds the sorted initial centres and is overwritten
 * (stays sorted); the midpoints are fp32 `0.5f * (c[j] + c[j+1])`; a value's label is the number of midpoints < it (so of
 * equal centres the first one takes the values); cluster sums are fp64; centre = (float)(sum / count); an empty cluster
 * keeps its centre; `iterations` steps, no convergence test.  ONE difference, which the k <= 256 entry keeps as it is:
 * between neighbouring floats c[j] < c[j+1] the rounded midpoint can be c[j+1] itself, which would label the value c[j+1]
 * with j; here such a midpoint is the float below c[j+1] instead, so every centre owns its own value and a codebook with
 * one centre per distinct value (k >= n: any small tensor at 16 bits) reproduces the values exactly and stays put.  In sorted order cluster j is the contiguous range of values
 * in (midpoint j-1, midpoint j], found by binary search, and its sum is taken piecewise (partial head, whole 1 024-value
 * blocks summed once before the loop, partial tail) in a fixed order: no atomics, deterministic -- two calls give
 * identical bits -- and within fp64 summation-order rounding of the unsorted form.  Replaces kmeans_quantization
 * (model_utils.py:73-76) where the writer asks for more than 8 bits.  Workspace from the caller
 * (lfgc_codec_kmeans_sorted_workspace_bytes; 0 for arguments the entry refuses), nothing allocated, no synchronisation. */
#define LFGC_CODEC_KMEANS_MAX_K 65536
int64_t lfgc_codec_kmeans_sorted_workspace_bytes(int64_t n, int k);
int lfgc_codec_kmeans1d_sorted_f32(const float* x_sorted, int64_t n, int k, float* centres, int iterations,
                                   void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);
/* labels[i] (uint16) = number of midpoints of the sorted `centres` (k <= 65 536) that are < x[i], the midpoints being those
 * of lfgc_codec_kmeans1d_sorted_f32 above; for values in any order. */
int lfgc_codec_labels_u16_f32(const float* x, int64_t n, int k, const float* centres, uint16_t* labels,
                              lfgc_stream_t stream);

/* Labels -> byte stream of the quantised blocks (ints_to_bits_to_bytes, model_utils.py:79-90): label i, masked to its low
 * `bits` bits, at stream bits [bits*i, bits*(i+1)), MSB first.  labels: uint8 (label_bytes 1, bits <= 8) or uint16
 * (label_bytes 2); 1 <= bits <= 16; packed_bytes >= (n*bits + 7) / 8, of which exactly that many are written.
 * TAIL: when n*bits is no multiple of 8 the leftover bits are LEFT-aligned in the last byte (plain continuation of the
 * stream, zero bits on the right).  The reference's helper right-aligns them, but its reader (and lfgc_codec_dequant_f32)
 * slices the stream MSB-first and repairs only the LAST label from the uint32 that follows the stream; at 1, 2, 3 and 5 bits
 * the last byte holds whole labels before the last one, which a right-aligned tail makes that reader mis-decode.  The
 * reference's writer only ever emits 8 bits (no tail), so there are no reference bytes to match -- only the reader's rule,
 * which the left-aligned tail satisfies at every width.  The file writer still appends the uint32. */
int lfgc_codec_pack_labels(const void* labels, int label_bytes, int64_t n, int bits, uint8_t* packed, int64_t packed_bytes,
                           lfgc_stream_t stream);

/* out[i] = centres[label_i], label_i = bits [bits*i, bits*(i+1)) of `packed`, MSB first, 1 <= bits <= 16
 * (read_in_data_quantized, model_utils.py:255-275). */
int lfgc_codec_dequant_f32(const uint8_t* packed, int64_t packed_bytes, int bits, int64_t n, const float* centres,
                           float* out, lfgc_stream_t stream);

/* Lossless entropy stage of the codec (the reference has none): byte-symbol rANS with a static order-0
 * model, interleaved over the 64 lanes of a wave.  Frequencies sum to M = 4096; the state x is 32 bits in [2^16, 2^32);
 * renormalisation moves one 16-bit word; the initial encoder state is 2^16.
 *   STREAM, little-endian:   u32 n | u16 R | u16 0 | u16 f[256] | u32 words[nc]   then per chunk   u32 state[64], u16 word[words[c]]
 *   with nc = ceil(n / 64R): 520 + 260 nc bytes of overhead.  A chunk is 64 R symbols, one wave; lane l codes the chunk
 *   positions 64 r + l, r = 0..R-1; a position at or beyond n is inactive in that round (no coding, no renormalisation).
 *   DECODER, r = 0..R-1, each active lane:  slot = x & 4095;  s = the symbol with cum[s] <= slot < cum[s] + f[s];
 *   x = f[s] (x >> 12) + slot - cum[s];  if x < 2^16: x = (x << 16) | next word -- the lanes that read in one round take
 *   consecutive words of the chunk in ascending lane order.  After the last round every state is 2^16 and the cursor stands at
 *   the end of the chunk's words.
 *   ENCODER, the inverse, r = R-1..0, each active lane:  if (x >> 20) >= f[s]: emit x & 0xFFFF, x >>= 16  (this form: f may be
 *   4096);  x = ((x / f[s]) << 12) + x mod f[s] + cum[s].  The words of round r lie in ascending lane order after those of the
 *   rounds below r.
 *   NORMALISATION of 256 counts h, n = sum h:  f[s] = 0 where h[s] = 0, else max(1, floor(4096 h[s] / n));  d = 4096 - sum f;
 *   walk the symbols cyclically by descending h (ties: ascending symbol), adding 1 to each visited symbol with h > 0 while
 *   d > 0, taking 1 from each visited symbol with f > 1 while d < 0, until d = 0;  cum[s] = sum of f below s.
 * 1 <= n < 2^32 and 1 <= rounds <= 65535, else LFGC_E_SHAPE.  Workspace from the caller (lfgc_codec_rans_workspace_bytes: 0
 * for arguments the entries refuse), 8-byte aligned; nothing allocated, no synchronisation, integer arithmetic only. */

/* counts[s] += the number of bytes of sym[0..n) equal to s (256 int64, 8-byte aligned, zeroed by the caller).  One LDS
 * histogram per wave flushed with integer atomics: deterministic. */
int lfgc_codec_histogram_u8(const uint8_t* sym, int64_t n, int64_t* counts, lfgc_stream_t stream);
/* HOST function (no device work): freq[256] from counts[256] by the rule above; counts >= 0 with 0 < sum <= 2^50. */
int lfgc_codec_rans_normalize_host(const int64_t* counts, uint16_t* freq);
int64_t lfgc_codec_rans_workspace_bytes(int64_t n, int rounds);
/* First pass: codes sym[0..n) with the device table freq[256] and keeps only the words per chunk, then scans them; the
 * workspace holds both for the second pass and *total_words (device int64) their sum: the stream has
 * 520 + 260 nc + 2 * total_words bytes. */
int lfgc_codec_rans_encode_count(const uint8_t* sym, int64_t n, int rounds, const uint16_t* freq, int64_t* total_words,
                                 void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);
/* Second pass, same arguments and the same workspace: codes again and writes the whole stream into out (2-byte aligned,
 * out_bytes >= 520 + 260 nc else LFGC_E_WORKSPACE), every chunk at its final place, the chunk's words filled from the end
 * backwards.  One writer per address, no atomics; a store is made only inside the chunk's own range and the buffer. */
int lfgc_codec_rans_encode_write(const uint8_t* sym, int64_t n, int rounds, const uint16_t* freq, uint8_t* out,
                                 int64_t out_bytes, void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);
/* out[0..n) = the symbols of the stream in[0..in_bytes) (4-byte aligned; n and rounds as its header says, which the caller
 * has read and checked: in_bytes >= 520 + 260 nc else LFGC_E_SHAPE).  Every word index is clamped to the chunk's own words
 * and every chunk to the buffer before a load, so no stream makes the kernel read outside in[0..in_bytes).  *status (device
 * int32, zeroed by the caller) |= 1 a lane wanted a word beyond its chunk, 2 a final state is not 2^16, 4 a chunk's cursor
 * did not end at its end, 8 a chunk does not lie inside the buffer. */
int lfgc_codec_rans_decode(const uint8_t* in, int64_t in_bytes, int64_t n, int rounds, uint8_t* out, int32_t* status,
                           void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);

/* The pruning mask once per CELL (mode 2 of the mask file; the reference has none).  A coefficient
 * tensor is viewed as x[c][j], c < C channels, j < S cells, in its flat order (x[c * S + j]); every drop layer multiplies it
 * by one factor per cell, so a pruned model's zero pattern is the same in all C channels.  The mask is then two streams: the
 * SUPPORT, one bit per cell (any channel non-zero), and the RESIDUAL, the mask bits of the support cells only, channel-major
 * over the compacted tensor V[c][r] = x[c][j_r] (j_r = the r-th support cell, ascending).  "Non-zero" is the rule of the
 * mask entry above: v != 0.0f, so -0.0 is zero and NaN is non-zero.  C >= 1, S >= 1 and C * S within int64, else
 * LFGC_E_SHAPE.  The two selections take the workspace of lfgc_codec_select_workspace_bytes for S elements, 8-byte
 * aligned.  Integer and copy work only; nothing allocated, no synchronisation, one writer per output address, no atomics. */

/* flags[j] = 1 where any channel of cell j is non-zero, else 0 (S bytes).  The one pass that reads the whole tensor: lanes
 * run over consecutive cells, 16-byte loads where S % 4 == 0, x is 16-byte and flags 4-byte aligned. */
int lfgc_codec_support_f32(const float* x, int C, int64_t S, uint8_t* flags, lfgc_stream_t stream);
/* bits[0 .. (n+7)/8): bit i (MSB first) = flags[i] != 0, tail bits zero.  The caller concatenates the flags of all tensors
 * first, so the stream needs no bit offsets on the write side. */
int lfgc_codec_pack_flags_u8(const uint8_t* flags, int64_t n, uint8_t* bits, lfgc_stream_t stream);
/* V[c * K + r] = x[c * S + j_r] over the K cells with flags[j] != 0, in ascending order; *count (device int64) = K.  V needs
 * room for C * K floats (C * S when K is not known beforehand).  The existing mask entry over V gives the residual bits, the
 * existing compaction over V the non-zero values of x in their flat order. */
int lfgc_codec_compact_support_f32(const float* x, int C, int64_t S, const uint8_t* flags, float* V, int64_t* count,
                                   void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);
/* The inverse: out[c * S + j] = support bit (bit_offset + j) ? V[c * K + rank of that bit among the set bits of
 * [bit_offset, bit_offset + j)] : 0, every element of out written.  0 <= K <= S comes from the file: every index into V is
 * clamped to C * K - 1 before the load (K = 0: nothing is loaded), so no file makes the kernel read outside V[0, C * K);
 * *status (device int32, zeroed by the caller) |= 1 where the S support bits hold a number of set bits other than K. */
int lfgc_codec_expand_support_f32(const uint8_t* support, int64_t bit_offset, int C, int64_t S, const float* V, int64_t K,
                                  float* out, int32_t* status, void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Error-bounded residual layer (the reference has none): what turns "the model's prediction p of a
 * voxel" into "a value within eps of the ground truth g".  Host side (file layout, rANS over the symbols, slab loop):
 * latent_feature_grid_compression_amd/model/residual_codec.py.  With eps a positive normal fp32 number, step = eps + eps and
 * inv = 1.0f / step formed on the host (LFGC_E_SHAPE unless all three are positive, normal and finite), per voxel, every
 * operation ONE fp32 rounding, never an fma:
 *     t = (g - p) * inv;   q = rintf(t)   (ties to even);   escape unless |q| <= 127   (NaN and Inf land here);
 *     r = p + (float)(int)q * step;       escape unless |(double)g - (double)r| <= (double)eps;
 *     symbol = (q << 1) ^ (q >> 31) in 0..254, or 255 for an escape.
 * A voxel with a symbol below 255 decodes to r, an escape to the bits of g (NaN payloads included), kept in lattice order.
 * The second test is the guarantee itself: the rounding of r breaks the bound for some voxels at small eps, and the test
 * makes those escape.  It holds for the decoder only if its p has the encoder's bits, so both sides form
 *     checksum = sum_i (uint64)bits(p_i) * (2 i + 1)  mod 2^64        (i = index in the array; integer adds, order-free)
 * and the caller compares them.  n >= 1; pred, gt, out, outliers 4-byte, checksum, counts and workspaces 8-byte aligned
 * (LFGC_E_ALIGN).  Nothing allocated, no synchronisation.
 * ---------------------------------------------------------------------------------------------- */

/* sym[i] = the symbol of voxel i; *checksum (device uint64, zeroed by the caller) += the checksum of pred.  One streaming
 * pass of 9 bytes per voxel: 4 voxels per lane (16-byte loads, one 4-byte store) where pred and gt are 16-byte and sym
 * 4-byte aligned, the n % 4 tail and any other alignment one voxel per lane. */
int lfgc_residual_quantize_f32(const float* pred, const float* gt, int64_t n, float eps, uint8_t* sym, uint64_t* checksum,
                               lfgc_stream_t stream);
/* Workspace of the two selections below (lfgc_codec_select_workspace_bytes' rule). */
int64_t lfgc_residual_workspace_bytes(int64_t n);
/* outliers[0..*count) = gt[i] of the voxels with sym[i] == 255, in order, bit for bit; count: device int64.  outliers needs
 * room for n floats where the count is not known beforehand. */
int lfgc_residual_outliers_f32(const uint8_t* sym, const float* gt, int64_t n, float* outliers, int64_t* count, void* workspace,
                               int64_t workspace_bytes, lfgc_stream_t stream);
/* out[i] = sym[i] == 255 ? outliers[rank of i among the escapes] : r(pred[i], sym[i]), every i < n written; out may be pred.
 * 0 <= K <= n is the caller's word for the number of outliers it holds (from the file; outliers may be NULL for K = 0): an
 * escape of rank >= K reads nothing, writes 0 and sets bit 1 of *status; bit 0 is set where the escapes found are not K
 * (*status: device int32, zeroed by the caller; *n_escape: device int64, the number found).  *checksum (zeroed by the
 * caller) += the checksum of pred, taken by a pass of its own before anything is written. */
int lfgc_residual_apply_f32(const float* pred, const uint8_t* sym, int64_t n, float eps, const float* outliers, int64_t K,
                            float* out, uint64_t* checksum, int64_t* n_escape, int32_t* status, void* workspace,
                            int64_t workspace_bytes, lfgc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused sample + Fourier-embed + MLP decoder
 * ---------------------------------------------------------------------------------------------- */

/* Shape of the decoder network (model/Feature_Grid_Model.py:37-48). */
typedef struct lfgc_mlp_desc {
    int32_t grid_channels;   /* C  = feature_grid.shape[0]                                   */
    int32_t hidden;          /* H  = hidden_channel                                           */
    int32_t num_layers;      /* L  = num_layer  (L hidden Linear+SnakeAlt, then final Linear) */
    int32_t n_freqs;         /* FourierEmbedding n_freqs (model/Feature_Embedding.py:20-34)   */
    int32_t d_in;            /* must be 3 */
    int32_t d_out;           /* must be 1 */
} lfgc_mlp_desc;

/* 1 if the compiled kernel set covers this shape: 1 <= C <= 32, 1 <= H <= 128, 1 <= L <= 8, n_freqs == 2, d_in 3, d_out 1
 * (every reference configuration and the NAS ranges of Multi_Objective_NAS.py:127-143); anything else is refused with
 * LFGC_E_UNSUPPORTED by the entry points below. */
int lfgc_mlp_supported(const lfgc_mlp_desc* desc);

/* Channel stride (floats) the sampler expects for the channel-last dense grid: C rounded up to 8. */
int lfgc_grid_channel_stride(int C);

/* Bytes of the packed-parameter blob and of the per-call stash (N samples) for this network. */
int64_t lfgc_packed_bytes(const lfgc_mlp_desc* desc);
int64_t lfgc_stash_bytes(const lfgc_mlp_desc* desc, int64_t n_samples);

/* Re-lay the nn.Linear parameters (weights[l] (out,in) row-major, biases[l] (out), l = 0..L with l = L
 * the final layer; host arrays of L+1 device pointers; named_parameters() order of
 * model/Feature_Grid_Model.py:43-48) into the blob the kernels read.  Run again whenever a parameter
 * changes.  `packed` device, >= lfgc_packed_bytes(), 16-byte aligned. */
int lfgc_pack_mlp_f32(const lfgc_mlp_desc* desc, const float* const* weights, const float* const* biases,
                      float* packed, lfgc_stream_t stream);

/* Where the sample positions come from. */
typedef struct lfgc_positions {
    const float* pos;        /* device (N,3) normalised positions, or NULL to generate the lattice below */
    int64_t n;               /* number of samples when pos != NULL */
    /* pos == NULL: full-volume lattice of visualization/OutputToVTK.py:11-37 (field_from_net), x-slab
     * [x_begin, x_end) of a (res0,res1,res2) volume cut into tiles of `tile` voxels; sample order =
     * row-major (x,y,z) of the slab, i.e. out[(x-x_begin)*res1*res2 + y*res2 + z].  Positions are formed
     * per tile exactly as the reference does (linspace(start,end,n) -> *2-1 -> *scales, fp32) from the ABSOLUTE voxel
     * index, so a slab may start and end anywhere, not only on tile boundaries. */
    int32_t res[3];
    int32_t x_begin, x_end;
    int32_t tile;            /* reference: 32 */
} lfgc_positions;

/* Arithmetic of the layer GEMMs inside lfgc_forward_f32 (inputs, outputs, accumulation and every other operation
 * are fp32 in both):
 *   LFGC_PRECISION_F32    v_mfma_f32_32x32x2_f32, bitwise an fp32 fmaf chain per output;
 *   LFGC_PRECISION_F16X2  every fp32 operand carried as an f16 pair hi + lo (22-24 significant bits), three
 *                         v_mfma_f32_32x32x16_f16 per product block with fp32 accumulation: same error level as the
 *                         fp32 build against the reference (fp32 summation order dominates), several times the
 *                         throughput.  Pre-activations are carried in turns of pi (weight images divided by pi at pack
 *                         time) and SnakeAlt is evaluated with the hardware cosine.  Valid while |pre-activations| <~ 800
 *                         and |grid features| < 65504; beyond that the affected outputs come out as NaN and *status is
 *                         set -- see lfgc_forward_f32.
 *   LFGC_PRECISION_F16    REDUCED precision (opt-in, never the default; does not meet the 1e-5 parity bound): weights and
 *                         activations of the layer GEMMs rounded to f16 (weights pre-scaled per layer as above), ONE
 *                         v_mfma_f32_32x32x16_f16 per product block, fp32 accumulation, fp32 master parameters, fp32
 *                         everything else.  This package's form of the "bf16 compute" BASELINE config 3 names (the
 *                         reference has no reduced-precision path): f16 rather than bf16 because it runs at the same
 *                         MFMA rate with 3 more mantissa bits and the ranges are known (scaled weights, activations
 *                         < 65504, gradients rescaled per tile).  Error ~1e-3 of the output range. */
#define LFGC_PRECISION_F32 0
#define LFGC_PRECISION_F16X2 1
#define LFGC_PRECISION_F16 2

/* forward().  Replaces model/Feature_Grid_Model.py:62-78 (everything after decode_volume):
 * F.grid_sample(bilinear, align_corners=False, zeros) of the dense grid (the cell arithmetic, shared with the backward:
 * csrc/lfgc_trilinear.h), Embedder.embed
 * (model/Feature_Embedding.py:14-16), torch.cat, L x (Linear + SnakeAlt), final Linear, optional
 * clamp(-1,1) (eval branch :78).
 *   grid_cl   device (D,H,W,Cs) channel-last dense grid, Cs = lfgc_grid_channel_stride(C)
 *   packed    device blob from lfgc_pack_mlp_f32
 *   out       device (N) fp32  (= the (N,1) result)
 *   stash     device, lfgc_stash_bytes(N) bytes, or NULL.  When given, the layer-0 input and every
 *             pre-activation are saved for lfgc_backward_f32 (private layout).
 *   status    device int32 or NULL (ignored by LFGC_PRECISION_F32).  The reference computes in fp32 and stays finite
 *             for any finite parameters (model/Feature_Grid_Model.py:12-13, :72-75); the f16 builds have a range.
 *             With status != NULL the call clears *status (a one-thread kernel), the f16 kernel sets it to 1 if any sample left that range,
 *             and the call then enqueues the same pass on the exact-fp32 build predicated on *status (its workgroups
 *             return immediately when it is 0): `out` (and `stash`) always hold reference-equivalent results, without
 *             a host synchronisation.  With status == NULL out-of-range samples are returned as NaN. */
int lfgc_forward_f32(const lfgc_mlp_desc* desc, const lfgc_positions* positions,
                     const float* grid_cl, int D, int H, int W,
                     const float* packed, int precision, int clamp, float* out, float* stash, int32_t* status,
                     lfgc_stream_t stream);

/* Backward of lfgc_forward_f32 (what autograd derives for model/Feature_Grid_Model.py:62-75;
 * triggered at training/training.py:137).  positions->pos must be non-NULL.
 *   precision   LFGC_PRECISION_* of the data-gradient chain dH_{l-1} = W_l^T dA_l and of the weight-gradient contraction
 *               dW_l = dA_l^T H_{l-1} (f16 builds: f16-split / single f16 products with fp32 accumulation; a tile whose
 *               inputs leave the f16 range takes the exact chain)
 *   stash       device, written by the forward call with the same inputs
 *   d_out       device (N)
 *   d_grid_cl   device (D,H,W,Cs)  ACCUMULATED into with float atomics (caller zeroes it)
 *   d_weights / d_biases  host arrays of L+1 device pointers, each OVERWRITTEN (same shapes as the
 *               parameters)
 *   d_pos       device (N,3) or NULL
 *   workspace   device scratch of lfgc_backward_workspace_bytes() bytes */
int64_t lfgc_backward_workspace_bytes(const lfgc_mlp_desc* desc, int64_t n_samples);
int lfgc_backward_f32(const lfgc_mlp_desc* desc, const lfgc_positions* positions,
                      const float* grid_cl, int D, int H, int W,
                      const float* packed, int precision, const float* stash, const float* d_out,
                      float* d_grid_cl, float* const* d_weights, float* const* d_biases, float* d_pos,
                      void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);

/* lfgc_backward_f32 with an ORDER-INDEPENDENT grid gradient: same arguments, same weight / bias / position gradients.
 * The feature gradients are scattered in 64-bit fixed point with integer atomics (one power-of-two quantum per call, taken
 * from max |feature gradient|; each contribution is rounded once, by at most half a quantum, which lies 2^-(61 - ceil(log2
 * (8 N))) below that maximum), so d_grid_cl is bitwise independent of the order of the samples and of the launch geometry.
 *   d_grid_cl   OVERWRITTEN, every element (no zero fill needed).  All zero if every feature gradient is zero.  If ANY
 *               feature gradient of the N samples is non-finite the WHOLE array is NaN (lfgc_backward_f32 poisons only
 *               the addresses that sample touches): a non-finite gradient never comes out finite.
 *   workspace   lfgc_backward_det_workspace_bytes(desc, N, D, H, W) bytes: lfgc_backward_f32's scratch + an int64
 *               accumulator of D H W Cs elements + the maximum word
 * N == 0 returns like lfgc_backward_f32 (zero weight / bias gradients, d_grid_cl untouched). */
int64_t lfgc_backward_det_workspace_bytes(const lfgc_mlp_desc* desc, int64_t n_samples, int D, int H, int W);
int lfgc_backward_det_f32(const lfgc_mlp_desc* desc, const lfgc_positions* positions,
                          const float* grid_cl, int D, int H, int W,
                          const float* packed, int precision, const float* stash, const float* d_out,
                          float* d_grid_cl, float* const* d_weights, float* const* d_biases, float* d_pos,
                          void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);
/* Host only: log2 of the quantum lfgc_backward_det_f32 uses for n_samples samples whose largest |feature gradient| has the
 * fp32 bit pattern max_bits: E - B with 2^E >= max (E minimal) and B = 61 - ceil(log2(8 n_samples)), so that the 8
 * n_samples contributions that can meet at one address sum to at most 2^61.  0 where no quantum is used (max_bits 0 or
 * non-finite, n_samples < 1). */
int lfgc_det_quantum_exp(uint32_t max_bits, int64_t n_samples);

/* Read-only launch-plan queries: which kernel build and launch shape lfgc_forward_f32 / lfgc_backward_f32 pick for these
 * arguments on the current device.  The launchers consume the very structs these entries fill (one selection function
 * each, csrc/lfgc_capi_forward.hip and csrc/lfgc_backward.hip), so a query cannot drift from a launch.  Nothing is
 * enqueued and no device pointer is read; the diagnostics environment knobs (LFGC_NO_ZRUN, LFGC_FWD_WAVES,
 * LFGC_WGRAD_NO_SPLIT) are honoured exactly as by the launch.  For tests and tools that must know which compiled
 * instantiation a shape reaches. */
typedef struct lfgc_forward_launch {
    int32_t resident;        /* 1: every layer block staged in LDS once; 0: streamed through a 2-deep ring     */
    int32_t waves;           /* waves per workgroup of the chosen build: 4 or 8                                 */
    int32_t coord_table;     /* lattice mode: per-axis coordinate tables held in LDS                           */
    int32_t zrun;            /* lattice mode, f16 builds: z-run tiles + column sampler                         */
    int32_t nzc;             /* z cells a z-run tile's column holds (2 when zrun == 0)                          */
    int32_t tiles_per_row;   /* z-run: ceil(res2 / 32), else 1                                                   */
    int32_t x2;              /* reserved: always 0                                                               */
    int32_t lds_bytes;       /* dynamic LDS of the launch                                                        */
    int64_t nbatches;        /* passes of one workgroup-sized batch of tiles                                     */
    int64_t ntiles;          /* z-run: tiles of the slab, else 0                                                 */
    int64_t grid;            /* workgroups launched                                                              */
} lfgc_forward_launch;

typedef struct lfgc_forward_plan_info {
    int32_t CH;              /* grid channels rounded up to 8: 8, 16, 24 or 32                                  */
    int32_t MT;              /* 32-row tiles of the hidden width (96 -> 128): 1, 2 or 4                         */
    int32_t has_redo;        /* 1: an f16 build with a status word -- `redo` describes the predicated launch    */
    int32_t reserved;
    lfgc_forward_launch first;   /* the launch of the build `precision` names                                   */
    lfgc_forward_launch redo;    /* the exact-fp32 range fallback behind it (zeroed when has_redo == 0)          */
} lfgc_forward_plan_info;

/* positions as for lfgc_forward_f32 (pos is only tested against NULL); has_stash / has_status: whether the launch would be
 * given a stash buffer / a status word.  Returns the LFGC_E_* the launch would return for the same shape arguments. */
int lfgc_forward_plan(const lfgc_mlp_desc* desc, const lfgc_positions* positions, int D, int H, int W, int precision,
                      int has_stash, int has_status, lfgc_forward_plan_info* out);

typedef struct lfgc_backward_plan_info {
    int32_t CH, MT;          /* as above                                                                         */
    int32_t waves;           /* waves per workgroup of the data kernel: 4 or 8                                  */
    int32_t nslabs;          /* partial slabs (tile groups) of the weight-gradient kernel                       */
    int32_t roles;           /* workgroups per tile group: 1, or L when the slab split is on                    */
    int32_t lds_bytes;       /* dynamic LDS of the data kernel                                                   */
    int64_t nbatches;        /* passes of the data kernel                                                        */
    int64_t grid;            /* workgroups of the data kernel (the weight-gradient kernel launches nslabs * roles) */
} lfgc_backward_plan_info;

int lfgc_backward_plan(const lfgc_mlp_desc* desc, int64_t n_samples, int precision, lfgc_backward_plan_info* out);

/* Gradient of the network output with respect to the sample positions, d out / d pos, and nothing else: what the
 * reference obtains by marking the positions requires_grad "for gradient calculation of nw" (training/training.py:99) and
 * differentiating model/Feature_Grid_Model.py:62-75 -- direct columns, Fourier embedding and grid_sample's coordinate
 * gradient -- without the parameter gradients lfgc_backward_f32 also produces.  Runs the data kernel of lfgc_backward_f32
 * in a build that writes no dstash, scatters nothing into a d_grid and is followed by no weight-gradient kernel; same
 * arithmetic per sample (the sampler's cell: csrc/lfgc_trilinear.h), same launch selection (lfgc_input_gradient_plan
 * reports it; nslabs and roles are 0).
 *   positions   positions->pos must be non-NULL (explicit list only, as the backward)
 *   stash       device, written by the lfgc_forward_f32 call with the same inputs
 *   d_out       device (N) upstream gradient, or NULL = ones: the gradient of the (unclamped) output itself
 *   d_pos       device (N,3), OVERWRITTEN
 * No workspace, nothing allocated, no synchronisation: graph-capturable like every other entry.  N == 0 returns LFGC_OK at
 * once.  Zero padding makes the sampler's part zero outside the grid, and the gradient jumps at cell faces. */
int lfgc_input_gradient_f32(const lfgc_mlp_desc* desc, const lfgc_positions* positions,
                            const float* grid_cl, int D, int H, int W,
                            const float* packed, int precision, const float* stash, const float* d_out,
                            float* d_pos, lfgc_stream_t stream);
int lfgc_input_gradient_plan(const lfgc_mlp_desc* desc, int64_t n_samples, int precision, lfgc_backward_plan_info* out);

/* The same for the channel-first wavelet levels: which kernel lfgc_idwt_level_drop_len_f32 (synthesis),
 * lfgc_idwt_level_drop_bwd_det_len_f32 (adjoint) and lfgc_dwt_level_len_f32 (forward DWT), and with them every entry that
 * forwards to these, launch for a shape.  One selection function per direction in csrc/lfgc_wavelet.hip fills this struct and
 * the launcher consumes it.  Pure host arithmetic: no device is needed. */
#define LFGC_WAVELET_TILED_DENSE     0   /* synthesis, 64-tap dense stencil (4 taps, taps == NULL)                    */
#define LFGC_WAVELET_TILED_SEPARABLE 1   /* synthesis, K + 1 staged planes per 2 output slices                        */
#define LFGC_WAVELET_SLIDING_WINDOW  2   /* synthesis, 4 taps separable, more than 40 000 output voxels per channel   */
#define LFGC_WAVELET_ANALYSIS_DENSE     3
#define LFGC_WAVELET_ANALYSIS_SEPARABLE 4
typedef struct lfgc_wavelet_plan_info {
    int32_t kernel;          /* LFGC_WAVELET_* above                                                             */
    int32_t drop;            /* 1: the DROP build (factors or penalty gradients folded in)                       */
    int32_t ki;              /* sliding window: planes-per-thread instantiation ceil(len / 256) = 1..3, else 0  */
    int32_t zchunk;          /* sliding window: output slices per workgroup, else 0                              */
    int32_t len;             /* staged plane offsets per z-plane                                                 */
    int32_t lds_bytes;       /* dynamic LDS of the launch                                                        */
    uint32_t grid[3];        /* workgroups: plane tiles, z tiles or chunks, channels                             */
} lfgc_wavelet_plan_info;

/* filter_len, C and extents as for the entry itself; has_taps: taps != NULL; has_drop: any of mul_lll / mul_hf given (the
 * adjoint: or penalty_grads[0] / [1]).  Returns the LFGC_E_* the launch would return for the same shape arguments
 * (LFGC_E_NULL only for out == NULL); *out is filled on LFGC_OK only. */
int lfgc_idwt_level_plan(int filter_len, int has_taps, int has_drop, int C, int d0, int d1, int d2, int t0, int t1, int t2,
                         lfgc_wavelet_plan_info* out);
int lfgc_idwt_level_bwd_plan(int filter_len, int has_taps, int has_drop, int C, int d0, int d1, int d2, int t0, int t1, int t2,
                             lfgc_wavelet_plan_info* out);
int lfgc_dwt_level_plan(int filter_len, int has_taps, int C, int n0, int n1, int n2, lfgc_wavelet_plan_info* out);

/* The same for the channel-last last level: which instantiation of its two kernels (csrc/lfgc_wavelet_cl.hip)
 * lfgc_idwt_level_cl_drop_len_f32 (synthesis) and lfgc_idwt_level_cl_drop_bwd_det_len_f32 (adjoint), and every entry
 * that forwards to them, launch for a shape.  One selection function per direction fills this struct and the launcher
 * consumes it.  A work item is (cells consecutive cells of the flattened (y,x) plane) x (cw channels) x (zchunk z steps);
 * items = ptiles * ngroups * nchunks, dealt to 8 queues of ceil(items / 8) workgroups: blocks = 8 ceil(items / 8). */
typedef struct lfgc_wavelet_cl_plan_info {
    int32_t cw;              /* channels per workgroup: 8, 16 (synthesis also 32)                                */
    int32_t cells;           /* plane cells per workgroup: 32 (adjoint: 32 or 64)                                */
    int32_t nt;              /* synthesis: 1 = streaming stores, else 0                                          */
    int32_t drop;            /* 1: the DROP build (factors or penalty gradients folded in)                       */
    int32_t zchunk;          /* z steps per work item (synthesis: of d0 + L/2 - 1 cell slices; adjoint: of d0)   */
    int32_t nchunks;         /* ceil(steps / zchunk)                                                             */
    int32_t ptiles;          /* ceil(plane cells / cells); synthesis plane (d1 + L/2 - 1)(d2 + L/2 - 1), adjoint d1 d2 */
    int32_t ngroups;         /* channel_stride / cw                                                              */
    int32_t threads;         /* 32 cw                                                                            */
    int32_t lds_bytes;       /* dynamic LDS of the launch (at most 80 KB)                                        */
    int32_t blocks;          /* workgroups                                                                       */
} lfgc_wavelet_cl_plan_info;

/* filter_len, C, channel_stride and extents as for the entry itself (taps given); has_drop: any of mul_lll / mul_hf given
 * (the adjoint: or penalty_grads[0] / [1]).  The z chunking minimises a cost that depends on the device's CU count:
 * num_cus > 0 is used as given, which makes the query pure host arithmetic with no device behind it; num_cus <= 0 means
 * the current device's count, which is what a launch uses.  The diagnostics switches LFGC_CL_CW, LFGC_CL_NT,
 * LFGC_CL_ADJ_NG and LFGC_CL_NCHUNKS are honoured as by a launch.  Returns the LFGC_E_* the launch would return for
 * the same shape arguments (LFGC_E_NULL only for out == NULL; C > 32 with has_drop: LFGC_E_UNSUPPORTED, which the drop
 * entries return for C > 32 whatever operands they are given); *out is filled on LFGC_OK only. */
int lfgc_idwt_level_cl_plan(int filter_len, int has_drop, int C, int channel_stride, int d0, int d1, int d2,
                            int t0, int t1, int t2, int num_cus, lfgc_wavelet_cl_plan_info* out);
int lfgc_idwt_level_cl_bwd_plan(int filter_len, int has_drop, int C, int channel_stride, int d0, int d1, int d2,
                                int t0, int t1, int t2, int num_cus, lfgc_wavelet_cl_plan_info* out);

/* The reduced-precision pair under the names SURVEY section 8(b) gives it (BASELINE config 3, "bf16 train step"; the
 * reference itself has no reduced-precision path): exactly lfgc_forward_f32 / lfgc_backward_f32 with precision =
 * LFGC_PRECISION_F16 -- layer GEMMs as single 16-bit products on the matrix pipe, fp32 accumulation, fp32 inputs, outputs
 * and master parameters.  The 16-bit format is IEEE f16, not bfloat16: the same MFMA rate on gfx950, 3 more mantissa bits.
 * What bfloat16 would have over it is fp32's exponent range; the forward entry therefore takes the same `status` word as
 * lfgc_forward_f32: with status != NULL a pass in which any sample left the f16 range (|pre-activation| >~ 800,
 * |grid feature| >= 65504) is redone on the exact-fp32 build, predicated on the word, in stream order -- `out` and
 * `stash` are then finite and reference-equivalent wherever the reference's are, as a bfloat16 path's would be finite.
 * With status == NULL such samples come out as NaN.  The backward needs no word: every tile of dA is rescaled by a power
 * of two before its conversion, and a weight-gradient tile whose activations leave the f16 range takes the exact MFMA. */
int lfgc_forward_bf16(const lfgc_mlp_desc* desc, const lfgc_positions* positions, const float* grid_cl, int D, int H, int W,
                      const float* packed, int clamp, float* out, float* stash, int32_t* status, lfgc_stream_t stream);
int lfgc_backward_bf16(const lfgc_mlp_desc* desc, const lfgc_positions* positions, const float* grid_cl, int D, int H, int W,
                       const float* packed, const float* stash, const float* d_out, float* d_grid_cl,
                       float* const* d_weights, float* const* d_biases, float* d_pos,
                       void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Ground-truth sampler and volume statistics
 * ---------------------------------------------------------------------------------------------- */

/* Training positions for flat voxel indices drawn on the device (IndexDataset.__getitem__, data/IndexDataset.py:90-96
 * with the index table of :56-57 and normalize_volume :7-8): raw (N,3) = integer lattice coordinates as fp32,
 * norm (N,3) = scales * (2 * ((raw - min_idx) / (max_idx - min_idx)) - 1), the reference's fp32 operations (bit-exact).
 *   flat device int64 (N), values in [0, X*Y*Z); res host int32[3]; min_idx / max_idx / scales host float[3]. */
int lfgc_lattice_positions_f32(const int64_t* flat, int64_t n, const int32_t* res, const float* min_idx,
                               const float* max_idx, const float* scales, float* raw, float* norm, lfgc_stream_t stream);

/* The same positions for indices DRAWN by the kernel itself (uniform with replacement, like the randint-on-device sampler
 * of SURVEY section 8 row f2): flat index i of draw `step` = floor(u * X*Y*Z / 2^64), u = first two words (hi, lo) of
 * Philox4x32-10 with counter (i lo, i hi, step lo, step hi) and key (seed lo, seed hi).
 *   state  device int64[2], zeroed ONCE by the caller: [0] = step, advanced by one per call ON THE DEVICE (a captured
 *          launch therefore draws a fresh batch on every graph replay), [1] = scratch, left at 0
 *   flat_out  device int64 (N) or NULL: the drawn indices
 * One launch instead of torch.randint + lfgc_lattice_positions_f32 (+ the generator bookkeeping of a graph replay). */
int lfgc_lattice_sample_f32(uint64_t seed, int64_t* state, int64_t n, const int32_t* res, const float* min_idx,
                            const float* max_idx, const float* scales, float* raw, float* norm, int64_t* flat_out,
                            lfgc_stream_t stream);

/* The (x_end - x_begin) * res1 * res2 normalised positions of the x-slab [x_begin, x_end) of the volume lattice, row-major
 * (x, y, z): the positions lfgc_forward_f32 forms for itself when positions->pos == NULL (same device function, same
 * per-tile arithmetic of visualization/OutputToVTK.py:23-37), written out for entries that take explicit positions only.
 *   res host int32[3] (each >= 2); tile >= 1 (reference: 32); scales host float[3] (dataset.scales); pos_out device (n,3). */
int lfgc_lattice_slab_positions_f32(const int32_t* res, int32_t x_begin, int32_t x_end, int32_t tile, const float* scales,
                                    float* pos_out, lfgc_stream_t stream);

/* trilinear_f_interpolation (data/Interpolation.py:8-44), bit-exact: fp32 lattice coordinates, fp64
 * alpha, fp32 lerps in x, y, z order without contraction.
 *   p device (N,3) raw positions; f device (X,Y,Z); min_bb/max_bb/res host float[3]; out device (N). */
int lfgc_gt_interp_f32(const float* p, const float* f, const float* min_bb, const float* max_bb,
                       const float* res, int64_t n, int X, int Y, int Z, float* out, lfgc_stream_t stream);

/* Ground truth and MSE of a train step in one pass (training/training.py:107-109 + nn.MSELoss, :127, :201):
 * gt as lfgc_gt_interp_f32 (bit-exact; also written to gt_out if non-NULL), loss (device float) = mean (pred - gt)^2 with
 * fp64 accumulation in a fixed order, d_pred (N) = 2 (pred - gt) / N = d loss / d pred.
 * workspace: lfgc_gt_mse_workspace_bytes(N) bytes. */
int64_t lfgc_gt_mse_workspace_bytes(int64_t n);
int lfgc_gt_mse_f32(const float* p, const float* f, const float* min_bb, const float* max_bb, const float* res,
                    int64_t n, int X, int Y, int Z, const float* pred, float* gt_out, float* d_pred, float* loss,
                    void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);

/* Partial sums for calculate_deviation_statistics (visualization/OutputToVTK.py:53-60):
 * acc[0] += sum (gt-pred)^2, acc[1] += sum |gt-pred|, acc[2] = min(acc[2], min gt), acc[3] = max(acc[3], max gt)
 * over n elements, fp64 accumulators on device (caller initialises acc = {0, 0, +inf, -inf}). */
int lfgc_deviation_partial_f32(const float* pred, const float* gt, int64_t n, double* acc, lfgc_stream_t stream);

/* Diagnostics: evaluates the kernels' own sin/cos (Cody-Waite + polynomial, lfgc_common.h) and SnakeAlt
 * on n device floats, fast path with the wave-level wide fallback exactly as the hot loops use them.
 * Lets the tests bound the transcendental error against fp64 without going through a network. */
int lfgc_debug_trig_f32(const float* x, int64_t n, float* sin_out, float* cos_out, float* snake_out,
                        lfgc_stream_t stream);

/* Diagnostics: the hardware v_sin_f32 path (fract(x / 2 pi) -> v_sin), NOT used by any kernel; kept so that the
 * accuracy argument for the polynomial path can be re-measured. */
int lfgc_debug_hwsin_f32(const float* x, int64_t n, float* out, lfgc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Direct volume rendering: the ray bookkeeping around the network evaluation.  Emission / absorption,
 * front to back, no scattering.  The values (and gradients) of the samples come from lfgc_forward_f32 /
 * lfgc_input_gradient_f32 between lfgc_ray_samples_f32 and lfgc_ray_composite_f32; the loop is host code
 * (visualization/Render.py).
 * All coordinates are the network's normalised coordinates (the volume's box is +-dataset.scales), directions are UNIT
 * vectors (not checked).  Per-ray arrays have R rows; `live` lists hold ray ids in [0, R) (not checked).  All arithmetic
 * is fp32 in exactly the stated order, no contraction, correctly rounded division.
 * ---------------------------------------------------------------------------------------------- */

/* Slab test of R rays against [box_min, box_max] (host float[3] each), axes a = 0, 1, 2 in this order, from tn = t_min,
 * tf = t_max:  d[a] == 0: the axis bounds nothing when box_min[a] <= o[a] <= box_max[a], else the ray misses;  otherwise
 * inv = 1/d[a], t1 = (box_min[a]-o[a])*inv, t2 = (box_max[a]-o[a])*inv, tn = fmaxf(tn, fminf(t1,t2)),
 * tf = fminf(tf, fmaxf(t1,t2)).  Hit iff tf > tn; n_steps = (int)ceilf((tf-tn)/dt), at most max_steps.
 * A miss writes n_steps = 0 and the empty interval t_near = t_far = t_min.
 *   origins, dirs device (R,3); t_near, t_far device (R); n_steps device int32 (R); t_min finite, dt > 0, max_steps >= 1. */
int lfgc_ray_clip_f32(const float* origins, const float* dirs, int64_t n_rays, const float* box_min, const float* box_max,
                      float t_min, float t_max, float dt, int max_steps, float* t_near, float* t_far, int32_t* n_steps,
                      lfgc_stream_t stream);

/* pos (n_live*S, 3): row j*S + s = sample k = k_next[ray] + s of ray = live[j].  S is a multiple of 32, so a 32-sample
 * tile of the forward kernel is 32 consecutive steps of one ray.  Segment k is [a, b] with a = tn + (float)k*dt and
 * b = fminf(a + dt, tf) -- the last segment of a ray is short, not missing --; the sample sits at tm = 0.5f*(a+b),
 * p = o + tm*d.  Rows with k >= n_steps repeat the ray's last valid sample (finite, inside the box); their value is never
 * used.  Rays of the list must have n_steps >= 1. */
int lfgc_ray_samples_f32(const int32_t* live, int64_t n_live, const float* origins, const float* dirs, const float* t_near,
                         const float* t_far, const int32_t* n_steps, const int32_t* k_next, float dt, int S, float* pos,
                         lfgc_stream_t stream);

/* Composite the S samples lfgc_ray_samples_f32 laid out for the same list into state (R,4) = premultiplied r, g, b and the
 * transmittance T per ray (initialised to (0,0,0,1) by the caller, updated in place; 16-byte aligned), then
 * k_next[ray] += S.  Rays outside the list are not touched.  A ray id may appear once in the list.
 *   values (n_live*S); grad (n_live*S, 3) or NULL; tf_table (K,4) = r, g, b, extinction per unit length (16-byte aligned),
 *   K >= 2; tf_scale = (K-1)/(v_max-v_min).
 * Per sample k < n_steps (later rows contribute nothing):
 *   len = fmaxf(b - a, 0) of its segment (a step count that the division rounded up puts the last a an ulp past t_far);
 *   u = fminf(fmaxf((v-v_min)*tf_scale, 0), K-1);  i = min((int)u, K-2);  f = u - i;
 *   rgba = tab[i] + f*(tab[i+1]-tab[i]);  alpha = 1 - expf(-rgba.w*len);
 *   shade = 1 without grad, else ka + kd*|g.d|/|g| when |g| > 0 (as fp32 computes it) and ka + kd otherwise: a headlight,
 *   two-sided diffuse;
 *   the sample contributes iff 1 - T_before < opacity_limit:  rgb += T*alpha*shade*rgba.rgb, then T *= 1 - alpha.
 * T never increases, so the contributing samples of a ray are a prefix; 32 samples at a time are folded by a product scan
 * and a tree sum, whose rounding differs from a sequential loop's by a few ulp per sample. */
int lfgc_ray_composite_f32(const int32_t* live, int64_t n_live, const float* values, const float* grad, const float* dirs,
                           const float* t_near, const float* t_far, const int32_t* n_steps, int32_t* k_next, float dt,
                           int S, const float* tf_table, int K, float v_min, float tf_scale, float opacity_limit, float ka,
                           float kd, float* state, lfgc_stream_t stream);

/* lfgc_ray_composite_f32 under a 2-D transfer function over the value and the gradient magnitude: the same lists, the same
 * state, segment length, alpha, shading, contribution rule, scan and sums -- the lookup is the only difference.
 *   grad (n_live*S, 3) REQUIRED, in the units the table's g axis is in (lfgc_input_gradient_f32: per unit of normalised
 *   position);  tf_table (Kv,Kg,4) row-major, entry tab[i*Kg + j] = r, g, b, extinction (16-byte aligned), Kv >= 2, Kg >= 2,
 *   Kv*Kg <= 2^22, read through the caches;  tf_scale = (Kv-1)/(v_max-v_min);  g_scale = (Kg-1)/g_max, finite and > 0: row j of
 *   the g axis sits at |g| = j*g_max/(Kg-1), the first at 0;  shade: 0 = no shading (shade = 1), 1 = the headlight with ka, kd.
 * Per sample k < n_steps, fp32, one rounding per operation, in this order:
 *   u  = fminf(fmaxf((v-v_min)*tf_scale, 0), Kv-1);  i = min((int)u, Kv-2);  f = u - i;
 *   gn = sqrtf((gx*gx + gy*gy) + gz*gz)                                   -- the |g| of the shading
 *   w  = fminf(fmaxf((gn-0)*g_scale, 0), Kg-1);      j = min((int)w, Kg-2);  h = w - j;
 *   lo = tab[i][j]   + f*(tab[i+1][j]   - tab[i][j]);
 *   hi = tab[i][j+1] + f*(tab[i+1][j+1] - tab[i][j+1]);
 *   rgba = lo + h*(hi - lo);
 * then as lfgc_ray_composite_f32.  A NaN value or gradient lands in row 0 of its axis (fmaxf), an infinite |g| in the last.
 * A table that does not depend on j gives lo == hi and with it the bits of lfgc_ray_composite_f32 on its (Kv,4) column.
 * Refused: LFGC_E_NULL for a missing pointer (grad included), LFGC_E_SHAPE for Kv < 2, Kg < 2, Kv*Kg > 2^22, a g_scale that
 * is not finite and positive, shade outside {0, 1} and the list errors of lfgc_ray_composite_f32. */
int lfgc_ray_composite2d_f32(const int32_t* live, int64_t n_live, const float* values, const float* grad, const float* dirs,
                             const float* t_near, const float* t_far, const int32_t* n_steps, int32_t* k_next, float dt,
                             int S, const float* tf_table, int Kv, int Kg, float v_min, float tf_scale, float g_scale,
                             int shade, float opacity_limit, float ka, float kd, float* state, lfgc_stream_t stream);

/* lfgc_ray_composite_f32 with pre-integrated classification (Engel, Kraus and Ertl 2001, in the integral-table form): what
 * is composited is not the segment around a sample under the table's value AT the sample, but the SLAB between two
 * consecutive samples under the table's mean over the value range the slab spans.  For a field that is linear between
 * samples the opacity is exact at any step.  Same lists, state, samples (lfgc_ray_samples_f32), shading, contribution
 * rule, scan and sums; fp32, one rounding per operation, in the stated order, unless said otherwise.
 *   pre device double (K,4), 16-byte aligned, K <= 2^22; tab and pre are read through the caches;
 *   carry_v device float (R), carry_k device int32 (R), initialised to -1 by the caller: the carry below.
 * Bracket.  Cell c of the 1-D table lies between rows c and c+1; along the cell fraction x in [0,1] both tau (column 3)
 * and the colour are linear.  For 0 <= x0 <= x1 <= 1, B(c; x0, x1) is the mean over [x0, x1] of (tau r, tau g, tau b, tau):
 * with t0 = tab[c], d = tab[c+1] - tab[c], s = x0 + x1, q = (x0*x0 + x0*x1) + x1*x1:
 *   B.w   = t0.w + (0.5f*d.w)*s
 *   B.rgb = (t0.w*t0.rgb + (0.5f*(t0.w*d.rgb + d.w*t0.rgb))*s) + (d.w*d.rgb)*(q/3)
 * (the integral over [x0, x1] is (x1-x0)*B; no cancellation where x0 is close to x1; at x0 == x1 the pointwise lookup).
 * pre[0] = 0, pre[i] = the sum over c < i of B(c; 0, 1), computed and stored in float64.
 * Slab mean of two table coordinates u_a, u_b (u as lfgc_ray_composite_f32 forms it; a NaN value lands in row 0): cell and
 * fraction of fminf(u_a,u_b) -> (i_lo, f_lo), of fmaxf(u_a,u_b) -> (i_hi, f_hi), i = min((int)u, K-2), f = u - i.
 *   i_lo == i_hi:  M = B(i_lo; f_lo, f_hi), tau_bar = M.w;
 *   otherwise:     M = ((1-f_lo)*B(i_lo; f_lo, 1) + (float)(pre[i_hi] - pre[i_lo+1])) + f_hi*B(i_hi; 0, f_hi), the difference
 *                  of the two rows taken in float64 and rounded once;  L = ((1-f_lo) + (float)(i_hi-i_lo-1)) + f_hi  (> 0:
 *                  f_lo < 1 whenever the cells differ);  tau_bar = M.w / L;
 *   c_bar = M.rgb / M.w where M.w > 0, else 0: the extinction-weighted mean colour.
 * A slab of length len has alpha = 1 - expf(-tau_bar*len) and the colour c_bar; it enters the ray as a sample does:
 * rgb += T*(alpha*shade)*c_bar, then T *= 1 - alpha.
 * Slabs of a ray.  Sample k < n_steps sits at t_m(k), the midpoint of its segment [a_k, b_k], and owns one slab:
 *   joined -- k > 0 and sample k-1 of the ray was composited (by this call or, through the carry, the one before):
 *             [t_m(k-1), t_m(k)], values (v_{k-1}, v_k), len = fmaxf(t_m(k) - t_m(k-1), 0);
 *   else the opening half slab [a_k, t_m(k)], values (v_k, v_k), len = fmaxf(t_m(k) - a_k, 0): k == 0 (a_0 = t_near) and
 *             the first sample after lfgc_ray_skip_f32 moved k_next.
 * Sample n_steps-1 also owns the closing half slab [t_m(k), b_k] (b_k = t_far), values (v_k, v_k),
 * len = fmaxf(b_k - t_m(k), 0), folded into the same lane after its own slab (alpha1, c1), with the sample's shade:
 *   e = (alpha1*shade)*c1 + (((1-alpha1)*alpha2)*shade)*c2, factor (1-alpha1)*(1-alpha2).
 * The slabs of a ray tile [t_near, t_far], so the image is continuous in dt.  shade is that of sample k.  A sample
 * contributes, its closing half included, iff 1 - T_before < opacity_limit.
 * Carry.  After a call carry_v[ray], carry_k[ray] hold the value and the step of the ray's last row with k < n_steps
 * (untouched where the call has none); on entry the carry is valid iff k_next[ray] > 0 and carry_k[ray] == k_next[ray] - 1.
 * Whoever moves k_next in between (lfgc_ray_skip_f32) thereby makes it stale and needs to do nothing else.
 * Refused before any launch: LFGC_E_NULL for a missing pointer except grad, LFGC_E_SHAPE for K < 2, K > 2^22 and the list
 * errors of lfgc_ray_composite_f32, LFGC_E_ALIGN for a tf_table, pre or state that is not 16-byte aligned. */
int lfgc_ray_composite_preint_f32(const int32_t* live, int64_t n_live, const float* values, const float* grad,
                                  const float* dirs, const float* t_near, const float* t_far, const int32_t* n_steps,
                                  int32_t* k_next, float dt, int S, const float* tf_table, int K, float v_min, float tf_scale,
                                  float opacity_limit, float ka, float kd, float* state, const double* pre, float* carry_v,
                                  int32_t* carry_k, lfgc_stream_t stream);

/* Joint histogram of value and gradient magnitude, the tool such a table is designed with:  counts[i*Bg + j] += the number
 * of the n samples whose cell is (i, j), where (i, j) is the cell lfgc_ray_composite2d_f32 interpolates in for a table of
 * (Bv+1, Bg+1) rows, by the same fp32 operations:  u = fminf(fmaxf((v-v_min)*v_scale, 0), Bv), i = min((int)u, Bv-1);
 * gn as above, w = fminf(fmaxf(gn*g_scale, 0), Bg), j = min((int)w, Bg-1).  Values outside the range and |g| above g_max fall
 * into the end bins, a NaN into bin 0 of its axis.
 *   values device (n); grad device (n,3); v_scale = Bv/(v_max-v_min); g_scale = Bg/g_max, both finite and > 0;
 *   counts device int64 (Bv,Bg), 8-byte aligned, ACCUMULATED into: the caller zeroes it once.
 * One LDS histogram of 32-bit counters per workgroup (Bv*Bg <= 16384, else LFGC_E_UNSUPPORTED), at most 2^31 + 256 rows per
 * workgroup, flushed with 64-bit integer atomics for the non-zero bins: the sums are integers, so the counts depend neither
 * on scheduling nor on how the samples are cut into calls.  n == 0 returns LFGC_OK at once. */
int lfgc_joint_histogram_f32(const float* values, const float* grad, int64_t n, int Bv, int Bg, float v_min, float v_scale,
                             float g_scale, int64_t* counts, lfgc_stream_t stream);

/* live_out[0..*count) = the rays r of prev[0..n_prev) (prev == NULL: r = 0..n_prev-1) with k_next[r] < n_steps[r] and
 * 1 - T[r] < opacity_limit, in the order of prev (ascending ids stay ascending: neighbouring pixels stay neighbours, and
 * the list does not depend on scheduling).  count: device int64.  live_out must not alias prev. */
int64_t lfgc_ray_compact_workspace_bytes(int64_t n);
int lfgc_ray_compact(const int32_t* prev, int64_t n_prev, const int32_t* n_steps, const int32_t* k_next, const float* state,
                     float opacity_limit, int32_t* live_out, int64_t* count, void* workspace, int64_t workspace_bytes,
                     lfgc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * First-hit isosurface ray casting: the surface {value == iso} seen along the rays, found by the same
 * march.  f(v) = v - iso;  inside(v) is f(v) >= 0, so a NaN is not inside.  Sample k of a ray sits at
 * t_m(k) = 0.5f*(a+b) of its segment [a, b], the position lfgc_ray_samples_f32 emits.  Per ray (R rows each, 16-byte
 * aligned, updated in place):
 *   state   (R,4): .x = the ray's last scanned value (the carry), .w = 1 while marching and 0 once bracketed, .y = .z = 0.
 *                  The caller initialises (0,0,0,1); lfgc_ray_compact with opacity_limit = 1 keeps exactly the marching rays.
 *   bracket (R,4): t_lo, t_hi, f_lo, f_hi.
 * ---------------------------------------------------------------------------------------------- */

/* Scan the S values lfgc_ray_samples_f32's rows were evaluated to (values (n_live*S), same list, same k_next).  Sample
 * k = k_next[ray] + s with 1 <= k < n_steps is a crossing iff inside(v[k-1]) != inside(v[k]); v[k-1] of the block's first
 * sample is the carry state.x, used only when k_next > 0.  Rows with k >= n_steps never cross.  At the FIRST crossing k of
 * the block:  bracket = (t_m(k-1), t_m(k), v[k-1]-iso, v[k]-iso), state = (v[k], 0, 0, 0), k_next = k.  Without one:
 * state = (value of the block's last row, 0, 0, 1), k_next += S.  Rays outside the list are not touched; a ray id may
 * appear once in the list. */
int lfgc_ray_iso_scan_f32(const int32_t* live, int64_t n_live, const float* values, const float* t_near, const float* t_far,
                          const int32_t* n_steps, int32_t* k_next, float dt, int S, float iso, float* state, float* bracket,
                          lfgc_stream_t stream);

/* One bisection step of the brackets of the n rays of `list`.  values (n) or NULL: the value at t_mid = 0.5f*(t_lo+t_hi) of
 * the bracket as it stands;  f = values[j] - iso;  (f >= 0) == (f_lo >= 0) ? (t_lo, f_lo) = (t_mid, f)
 * : (t_hi, f_hi) = (t_mid, f).  Then (at once when values is NULL) pos row j = o + t_mid*d with t_mid = 0.5f*(t_lo+t_hi) of
 * the updated bracket: the next trial.  pos (n,3). */
int lfgc_ray_iso_refine_f32(const int32_t* list, int64_t n, const float* values, const float* origins, const float* dirs,
                            float iso, float* bracket, float* pos, lfgc_stream_t stream);

/* q = f_lo/(f_lo - f_hi);  t = t_lo + (t_hi - t_lo)*q, the midpoint 0.5f*(t_lo+t_hi) when q is not finite;
 * t_hit[j] = fminf(fmaxf(t, t_lo), t_hi);  pos row j = o + t_hit*d.  The two ends differ in inside(), so f_lo != f_hi.
 * t_hit (n), pos (n,3): rows of the list, not of the rays. */
int lfgc_ray_iso_finish_f32(const int32_t* list, int64_t n, const float* origins, const float* dirs, const float* bracket,
                            float* t_hit, float* pos, lfgc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Isosurface triangle meshes: marching tetrahedra on the Kuhn triangulation of the volume lattice, one
 * x-slab at a time.  The loop is host code (visualization/Mesh.py): values of the slab (lfgc_forward_f32 in lattice mode)
 * -> count -> read the two totals -> emit -> lfgc_ray_iso_refine_f32 / lfgc_ray_iso_finish_f32 on the emitted brackets
 * with list = 0..n-1.
 *   values  device (nx, ny, nz), z contiguous: nx consecutive x-planes of the lattice, of which the first n_owner are the
 *           slab's OWNER planes.  A slab with owner planes [x0, x1) of a volume of X planes is given the planes
 *           [x0, min(x1 + 2, X)): planes beyond the ones passed must be beyond the volume.  1 <= n_owner <= nx; ny, nz >= 2;
 *           nx*ny*nz <= 2^27 (else LFGC_E_UNSUPPORTED).
 *   inside(v) is v - iso >= 0 in fp32 (v == iso is inside, a NaN is not), as in the ray caster.
 *   Edges: type ty = 1..7 with offset o = (ty>>2 & 1, ty>>1 & 1, ty & 1) in (x, y, z).  Edge (p, ty) joins its owner p to
 *           p + o, exists when p + o is a lattice point, and carries a mesh vertex when inside() differs at its ends.
 *           Vertices are ordered by ascending (x, y, z, ty) of the owner.
 *   Cells:  (x, y, z) with x < X-1 etc. hold six tetrahedra, one per permutation pi of (0,1,2) in lexicographic order:
 *           corners w0 = (0,0,0), w1 = w0 + e[pi0], w2 = w1 + e[pi1], w3 = (1,1,1).  With m = the 4-bit inside mask of
 *           (w0..w3): one corner a alone on its side, the others b < c < d: triangle (ab, ac, ad); two inside a < b, two
 *           outside c < d: (ac, ad, bd) then (ac, bd, bc); xy = the vertex on the edge between corners x and y.  A triangle
 *           whose normal (q1-q0) x (q2-q0), taken at the edge midpoints of the unit cube, does not point from the centroid of
 *           the inside corners to that of the outside corners has its second and third vertex swapped: normals point out of
 *           {v >= iso}.  Triangles are ordered by cell (x, y, z), then tetrahedron, then as listed.
 * The result does not depend on how the volume is cut into slabs.  No atomics: two runs give the same bits.
 * ---------------------------------------------------------------------------------------------- */

/* Bytes of workspace for a slab of these extents (16 for extents the entries refuse). */
int64_t lfgc_iso_mesh_workspace_bytes(int32_t nx, int32_t n_owner, int32_t ny, int32_t nz);

/* Classify the points of the planes [0, min(n_owner+1, nx)) (7-bit crossing-edge flag) and the cells below the planes
 * [0, min(n_owner, nx-1)) (0..12 triangles) and leave both and their exclusive prefix sums in the workspace (16-byte
 * aligned), for lfgc_iso_mesh_emit_f32.  totals device int64[2]: [0] the vertices owned by the owner planes, [1] the
 * triangles of the cells whose lowest corner lies in them. */
int lfgc_iso_mesh_count_f32(const float* values, int32_t nx, int32_t n_owner, int32_t ny, int32_t nz, float iso,
                            int64_t* totals, void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);

/* After lfgc_iso_mesh_count_f32 with the same values, extents, iso and workspace.  Per owned crossing edge, in order, row j:
 *   origins (n,3) = P(p) = (xs[x], ys[y], zs[z]);  dirs (n,3) = P(p+o) - P(p) per component (not unit vectors);
 *   bracket (n,4) = (0, 1, v(p) - iso, v(p+o) - iso), 16-byte aligned: the vertex is what lfgc_ray_iso_finish_f32 makes of it.
 * Per triangle, in order, three int32 vertex indices vertex_base + rank, where the ranks count this slab's vertices from 0
 * and run on into the plane after the owner planes (the next slab's first vertices, when it starts at that plane with
 * vertex_base + totals[0] as its base).  The caller keeps vertex_base + the slab's ranks below 2^31.
 *   xs device (nx): the slab's planes; ys device (ny); zs device (nz).  n_vertices, n_triangles: rows of the outputs, the
 *   totals of the count; rows past them are not written; both 0 returns at once. */
int lfgc_iso_mesh_emit_f32(const float* values, int32_t nx, int32_t n_owner, int32_t ny, int32_t nz, float iso,
                           const float* xs, const float* ys, const float* zs, int64_t vertex_base,
                           const void* workspace, int64_t workspace_bytes, int64_t n_vertices, int64_t n_triangles,
                           float* origins, float* dirs, float* bracket, int32_t* triangles, lfgc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Empty-space skipping for the direct volume renderer.  The volume lattice has res = (X, Y, Z) points
 * and cells = res - 1 per axis.  Bricks have an edge of B >= 1 cells: nb_a = ceil(cells_a / B) per axis, brick i of an axis
 * holds the lattice points i B .. min((i+1) B, res-1) inclusive, so a face plane belongs to both neighbours.  Tables are
 * row-major (nbx, nby, nbz).  No atomics, one writer per brick and per ray: two runs give the same bits.
 * ---------------------------------------------------------------------------------------------- */

/* Fold the lattice values of the planes [x_begin, x_end) (values device (x_end-x_begin, Y, Z), z contiguous) into
 * minmax device (nbx, nby, nbz, 2) fp32 = (min, max), 8-byte aligned, which the caller initialises to (+inf, -inf): every
 * brick that holds one of the slab's planes is folded with those of its points that the slab holds; the others are not
 * touched.  A NaN makes its bricks (-inf, +inf).  Launches are stream-ordered and min / max are exact, so the table does
 * not depend on how the volume is cut into slabs, and the volume need not be resident.
 *   res host int32[3], each >= 2; 0 <= x_begin < x_end <= X. */
int lfgc_brick_minmax_f32(const float* values, const int32_t* res, int32_t x_begin, int32_t x_end, int32_t B, float* minmax,
                          lfgc_stream_t stream);

/* occ[b] (device uint8, n_bricks) = 0 iff the brick is empty under the transfer function, else 1.  With lo = min - margin,
 * hi = max + margin and u(v) = fminf(fmaxf((v-v_min)*tf_scale, 0), K-1) -- lfgc_ray_composite_f32's expression, tf_scale the
 * float it is given -- the brick is empty iff the extinction tab[i].w is zero for every row i = floorf(u(lo)) ..
 * ceilf(u(hi)).  u is monotone in fp32, so every value in [lo, hi] interpolates between rows of that range: the composite
 * kernel gives such a sample the extinction 0 exactly.
 *   minmax device (n_bricks, 2), 8-byte aligned; tf_table (K,4), 16-byte aligned, K >= 2; margin >= 0. */
int lfgc_brick_occupancy_f32(const float* minmax, int64_t n_bricks, const float* tf_table, int K, float v_min, float tf_scale,
                             float margin, uint8_t* occ, lfgc_stream_t stream);

/* For every ray of live[0..n_list) (live == NULL: the rays 0..n_list-1), while k_next < n_steps: look at the samples
 * k = k_next .. min(k_next + S, n_steps) - 1 at lfgc_ray_samples_f32's positions, operation for operation (segment [a, b],
 * tm = 0.5f*(a+b), p = o + tm*d).  Per axis q = (p - box_min)/(box_max - box_min)*(float)cells, one rounding per operation,
 * c_lo = (int)fminf(fmaxf(floorf(q - g), 0), cells-1) and c_hi the same with q + g; the sample touches the bricks
 * {c_lo/B, c_hi/B} of each axis, at most 8.  The guard g = 1/16 cell covers the rounding difference between this q and the
 * index coordinate the samplers form for themselves (lfgc_gt_interp_f32, the forward kernel's grid lookup) for up to 2^16
 * lattice points per axis.  If no sample of the block touches a brick with occ != 0: k_next += S, skipped[ray] += 1, and
 * again; otherwise the ray is left there.  k_next only moves in multiples of S, so the blocks that follow hold the rows they
 * would have held anyway.  Neither state nor a ray outside the list is touched; a ray id may appear once in the list.
 *   box_min < box_max host float[3]; cells host int32[3], each >= 1; occ device uint8 (nbx, nby, nbz); skipped device
 *   int32 (R), zeroed by the caller; S a multiple of 32. */
#define LFGC_RAY_SKIP_GUARD 0.0625f          /* the guard g above, in cells */
int lfgc_ray_skip_f32(const int32_t* live, int64_t n_list, const float* origins, const float* dirs, const float* t_near,
                      const float* t_far, const int32_t* n_steps, int32_t* k_next, float dt, int S, const float* box_min,
                      const float* box_max, const int32_t* cells, int32_t B, const uint8_t* occ, int32_t* skipped,
                      lfgc_stream_t stream);

/* ----------------------------------------------------------------------------------------------
 * Structural similarity (SSIM) of two fp32 arrays a, b of shape (n0, n1, n2), row-major, axis 0 slowest.
 * Axis a has a window of w_a taps (1..16) with fp64 weights g_a[0..w_a) that the caller has normalised to sum 1, and a
 * stride s_a >= 1.  Windows are valid-only: m_a = (n_a - w_a) / s_a + 1 of them, window (i0,i1,i2) covers
 * i_a s_a <= idx_a < i_a s_a + w_a.  With W(t) = g0[t0] g1[t1] g2[t2] the moments mu_x, mu_y, E_xx, E_yy, E_xy are the
 * W-weighted sums of x, y, x x, y y, x y in fp64 (x from a, y from b; a product of two fp32 values is exact in fp64), and
 *   vx = k (E_xx - mu_x mu_x)   vy = k (E_yy - mu_y mu_y)   vxy = k (E_xy - mu_x mu_y)          k = cov_norm
 *   SSIM = ((2 mu_x mu_y + c1)(2 vxy + c2)) / ((mu_x mu_x + mu_y mu_y + c1)(vx + vy + c2))
 * The three second moments take the same operation sequence, so two buffers of equal contents give exactly 1.0 in every
 * window.  A NaN stays in the windows that cover it.
 *   plane_sums device double (m0): plane_sums[i0] = the sum of the SSIM of the windows (i0, ., .), added in an order that
 *              depends on (n1, n2, w, s) only -- not on n0, not on the launch: a call on the sub-array a[x0:x1] gives the
 *              planes it holds the same bits as a call on the whole array.  No floating-point atomics.
 *   map        device double (m0, m1, m2) or NULL.
 *   weights    host, w[0] + w[1] + w[2] finite values, axis 0 first; w, s host int[3].  c1, c2, cov_norm positive, finite.
 *   workspace  lfgc_ssim_workspace_bytes(n0, n1, n2, w, s) bytes, 8-byte aligned: one double per workgroup.
 * Decided before anything is launched: LFGC_E_NULL for a missing pointer other than map; LFGC_E_SHAPE for n_a < w_a,
 * w_a < 1, s_a < 1, a non-finite weight or a c1, c2, cov_norm that is not positive and finite; LFGC_E_UNSUPPORTED for
 * w_a > 16, n0 n1 n2 > 2^61 and more than 2^31 - 1 workgroups (m0 times the tiles of a plane, 8 x 32 windows each for
 * overlapping windows); LFGC_E_WORKSPACE for a short workspace; LFGC_E_ALIGN for plane_sums, map or workspace not 8-byte
 * aligned.  Nothing allocated, no synchronisation.  lfgc_ssim_workspace_bytes returns 0 for refused arguments.
 * ---------------------------------------------------------------------------------------------- */
int64_t lfgc_ssim_workspace_bytes(int n0, int n1, int n2, const int* w, const int* s);
int lfgc_ssim_planes_f32(const float* a, const float* b, int n0, int n1, int n2, const double* weights, const int* w,
                         const int* s, double c1, double c2, double cov_norm, double* plane_sums, double* map,
                         void* workspace, int64_t workspace_bytes, lfgc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LFGC_H */
