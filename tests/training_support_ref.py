"""numpy references of the small kernels that run around every training step (csrc/lfgc_drop.hip, csrc/lfgc_misc.hip):
the penalty sums and gradients, the stand-alone drop layer, the slice fold, the fused MSE, the deviation statistics and the
lattice sampler's draw, each stated in the precision its tolerance is derived for, plus the seeded inputs both test modules
share.  Test infrastructure: pinned by tests/test_training_support_host.py, used by tests/test_training_support_gpu.py."""
import math

import numpy as np

from philox_ref import philox4x32_10

L1, L2, DKL = 0, 1, 2                                   # LFGC_PENALTY_* of include/lfgc.h
KIND_NAMES = {L1: 'l1', L2: 'l2', DKL: 'dkl'}
# Molchanov et al.'s constants as the reference multiplies them into fp32 tensors: fp32 values, widened
K1, K2, K3 = (float(np.float32(v)) for v in (0.63576, 1.87320, 1.48695))

ULP32 = 2.0 ** -23                                      # one fp32 ulp, relative
DENORM32 = 2.0 ** -149                                  # the smallest fp32 denormal

SUM_SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 4097, 1 << 20, (1 << 20) + 1, (1 << 20) + 1025]
GRAD_SIZES = [1, 255, 256, 257, 524288, 524289, 524288 + 257]
# log alpha = log_var - 2 log_theta of the appended pairs: both softplus branches, the sigmoid's saturation on either side,
# the last normal and the overflowing exponents.  20 and 24 are where 1 - sigmoid still matters to the gradient but no
# longer survives being formed as a difference in fp64 (see dkl_grad).
DKL_LOG_ALPHAS = [1e-3, -1e-3, 0.0, 30.0, -30.0, 100.0, -100.0, -478.0, 700.0, -700.0, 1e4, -1e4, 20.0, 24.0]
SPECIALS = [-0.0, 1e-40]                                # -0.0; an fp32 denormal
HUGE = [3e19, -3e19]                                    # 3e19^2 overflows fp32: the sum has to be taken in fp64


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).reshape(-1).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).reshape(-1).view(np.uint64)


# ---- 1. penalties --------------------------------------------------------------------------------------------------------

def penalty_inputs(kind, n, seed=0, huge=False):
    """(a, b) fp32 of one term: b is None but for DKL.  L1 / L2: normal draws with every 17th element exactly 0 and, from
    the end backwards, as many of SPECIALS as fit beside one draw -- a sum of order n, against which an ordinary element
    lost or rounded in fp32 shows.  With `huge`, HUGE in front of them: the same tensor with +-3e19 in it, whose sum
    (6e19, or 1.8e39 for L2) hides everything else and shows only that the accumulator is fp64.  DKL: log_thetas ~ N(0, 0.5),
    log_var ~ N(0, 4) and, at the end, as many pairs (0, la) / (-la/2, 0) of DKL_LOG_ALPHAS as fit."""
    rng = np.random.default_rng(1000 * kind + n + 7919 * seed)
    if kind != DKL:
        a = rng.standard_normal(n).astype(np.float32)
        a[16::17] = 0.0
        tail = (HUGE if huge else []) + SPECIALS
        k = min(len(tail), n - 1)
        if k:
            a[n - k:] = np.asarray(tail[len(tail) - k:], np.float32)
        return a, None
    assert not huge
    a = rng.normal(0.0, 0.5, n).astype(np.float32)
    b = rng.normal(0.0, 4.0, n).astype(np.float32)
    k = min(len(DKL_LOG_ALPHAS), n - 1)
    for j, la in enumerate(DKL_LOG_ALPHAS[:k]):
        i = n - k + j
        if j % 2 == 0:
            a[i], b[i] = 0.0, la                        # la = b
        else:
            a[i], b[i] = -la / 2.0, 0.0                 # la = -2a
    return a, b


def _log_alpha(a, b, dtype):
    return np.asarray(b, np.float32).astype(dtype) - dtype(2.0) * np.asarray(a, np.float32).astype(dtype)


def penalty_values(kind, a, b=None, dtype=np.float64):
    """The terms of include/lfgc.h's formulas, per element, in `dtype` (fp64, or long double for the host check)."""
    a64 = np.asarray(a, np.float32).astype(dtype)
    if kind == L1:
        return np.abs(a64)
    if kind == L2:
        return a64 * a64
    la = _log_alpha(a, b, dtype)
    k1, k2, k3 = dtype(K1), dtype(K2), dtype(K3)
    with np.errstate(over='ignore'):
        t1 = k1 / (dtype(1.0) + np.exp(-(k2 + k3 * la)))
        t2 = dtype(0.5) * np.where(la < 0, -la + np.log1p(np.exp(np.minimum(la, 0))), np.log1p(np.exp(-np.maximum(la, 0))))
    return -t1 + t2 + k1


def penalty_sum64(kind, a, b=None):
    """The exactly rounded fp64 sum of the fp64 terms."""
    return math.fsum(penalty_values(kind, a, b).tolist())


def penalty_sum(kind, a, b=None):
    """math.fsum of the fp64 terms, rounded once to fp32 (an L2 term holding 3e19 rounds to +inf: its square alone is
    beyond fp32, so that case is read in fp64, through the C-ABI)."""
    with np.errstate(over='ignore'):
        return np.float32(penalty_sum64(kind, a, b))


def dkl_dla(a, b, dtype=np.float64):
    """d/d(la) of -k1 sigmoid(k2 + k3 la) + 0.5 softplus(-la) = -k1 k3 sigmoid'(x) - 0.5 sigmoid(-la), x = k2 + k3 la, with
    sigmoid'(x) = e / (1 + e)^2, e = exp(-|x|): the product s (1 - s) written without forming 1 - s as a difference, which
    in fp64 is exact to 2^-53 absolute only -- at la = 24 the other term has sunk to 2e-11 and the product to 5e-17, so the
    difference form is wrong by 2.4e-6 of the gradient there (fp32 torch's own autograd far more, earlier)."""
    la = _log_alpha(a, b, dtype)
    k1, k2, k3 = dtype(K1), dtype(K2), dtype(K3)
    with np.errstate(over='ignore', under='ignore'):
        e = np.exp(-np.abs(k2 + k3 * la))
        return -k1 * k3 * (e / ((dtype(1.0) + e) * (dtype(1.0) + e))) - dtype(0.5) / (dtype(1.0) + np.exp(la))


def dkl_dla_difference_form(a, b, dtype=np.float64):
    """The same derivative with s (1 - s) formed literally: what a kernel computing 1 - s gives.  Host check only."""
    la = _log_alpha(a, b, dtype)
    k1, k2, k3 = dtype(K1), dtype(K2), dtype(K3)
    with np.errstate(over='ignore', under='ignore'):
        s = dtype(1.0) / (dtype(1.0) + np.exp(-(k2 + k3 * la)))
        return -k1 * k3 * s * (dtype(1.0) - s) - dtype(0.5) / (dtype(1.0) + np.exp(la))


def penalty_grads(kind, a, b, g, dtype=np.float64):
    """(grad_a, grad_b) for the upstream weight g (fp32).  L1, L2: fp32, the kernel's own operations (bit for bit).
    DKL: `dtype`, unrounded (grad_b = g d_la, grad_a = -2 g d_la)."""
    g = np.float32(g)
    a = np.asarray(a, np.float32)
    if kind == L1:
        return g * ((a > 0).astype(np.int32) - (a < 0).astype(np.int32)).astype(np.float32), None      # sign(-0.0) = +0.0
    if kind == L2:
        with np.errstate(over='ignore'):
            return g * (np.float32(2.0) * a), None
    d = dkl_dla(a, b, dtype)
    return dtype(g) * (dtype(-2.0) * d), dtype(g) * d


def dkl_grad_bound(ref):
    return ULP32 * np.abs(np.asarray(ref, np.float64)) + DENORM32


# ---- 3. stand-alone drop layer -------------------------------------------------------------------------------------------

def drop_inputs(C, n, thr, seed=0):
    """x (C, n), mul (n), g (C, n) fp32.  The factors straddle the threshold: values equal to it, one ulp below it, a NaN."""
    rng = np.random.default_rng(31 * C + n + 7919 * seed)
    x = rng.standard_normal((C, n)).astype(np.float32)
    g = rng.standard_normal((C, n)).astype(np.float32)
    mul = rng.uniform(0.0, 1.0, n).astype(np.float32)
    t = np.float32(0.5 if thr is None else thr)
    edge = [t, np.nextafter(t, np.float32(0.0)), np.float32(np.nan), np.nextafter(t, np.float32(1.0)), np.float32(0.0), -t]
    for j, v in enumerate(edge[:n]):
        mul[(j * 43) % n] = v                           # n = 1: the factor equal to the threshold
    return x, mul, g


def drop_value(x, mul, thr):
    """drop_value of csrc/lfgc_drop_value.h in fp32 numpy, op for op: x*m, or with a threshold (x*hard - x*m) + x*m."""
    x, m = np.asarray(x, np.float32), np.asarray(mul, np.float32)[None, :]
    with np.errstate(invalid='ignore'):
        soft = x * m
        if thr is None:
            return soft
        hard = (m >= np.float32(thr)).astype(np.float32)
        return (x * hard - soft) + soft


def drop_grads(x, mul, g):
    """d_x = g*m in fp32 (bit for bit); d_mul = sum_c g*x in fp64 with its bound C 2^-24 sum_c |g x| (an FMA chain of C
    steps: one rounding per step, each of a partial sum no larger than sum |g x|)."""
    x, m, g = np.asarray(x, np.float32), np.asarray(mul, np.float32), np.asarray(g, np.float32)
    with np.errstate(invalid='ignore'):
        d_x = g * m[None, :]
    p = g.astype(np.float64) * x.astype(np.float64)
    return d_x, p.sum(0), x.shape[0] * 2.0 ** -24 * np.abs(p).sum(0)


# ---- 4. slice fold ---------------------------------------------------------------------------------------------------------

def sum_slices(slices, nslices, stride, n):
    """((s0 + s1) + s2) + ... in fp32, slice s at slices[s*stride : s*stride + n]."""
    slices = np.asarray(slices, np.float32)
    acc = slices[:n].copy()
    for s in range(1, nslices):
        acc = acc + slices[s * stride:s * stride + n]          # fp32 + fp32 -> one rounding
    return acc


# ---- 5. fused MSE ----------------------------------------------------------------------------------------------------------

def mse_reference(pred, gt):
    """(d_pred bit for bit, loss to one fp32 ulp) of lfgc_gt_mse_f32 for a given ground truth."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    n = pred.size
    d32 = pred - gt
    d_pred = d32 * np.float32(2.0 / n)
    loss = np.float32(math.fsum((d32.astype(np.float64) ** 2).tolist()) / n)
    return d_pred, loss


# ---- 6. deviation statistics -------------------------------------------------------------------------------------------------

def deviation(pred, gt):
    """[sum d^2, sum |d|, min gt, max gt] in fp64 with d = gt - pred in fp32; the sums exactly rounded."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    d = (gt - pred).astype(np.float64)
    return np.array([math.fsum((d * d).tolist()), math.fsum(np.abs(d).tolist()), float(gt.min()), float(gt.max())], np.float64)


# ---- 7. lattice sampler ------------------------------------------------------------------------------------------------------

def lattice_draw(n, step, seed, n_voxels):
    """The flat indices lfgc_lattice_sample_f32 documents: Philox4x32-10 with counter (i lo, i hi, step lo, step hi) and key
    (seed lo, seed hi); u64 = word 0 (high) and word 1 (low); floor(u64 * n_voxels / 2^64) in Python integers."""
    ctr = np.zeros((n, 4), np.uint32)
    i = np.arange(n, dtype=np.uint64)
    ctr[:, 0] = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (i >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2] = step & 0xFFFFFFFF
    ctr[:, 3] = (step >> 32) & 0xFFFFFFFF
    r = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32))
    return np.array([(((int(hi) << 32) | int(lo)) * int(n_voxels)) >> 64 for hi, lo in zip(r[:, 0], r[:, 1])], np.int64)


def lattice_flat_indices(res, seed=0):
    """The flat indices of section 7 for a lattice `res`: both ends, the 2^31 and 2^32 boundaries where in range, row and
    plane boundaries and their neighbours, 10 000 random ones."""
    X, Y, Z = (int(v) for v in res)
    nv = X * Y * Z
    rng = np.random.default_rng(nv % 100003 + seed)
    pts = [0, nv - 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32]
    for k in (1, 2, Y - 1, Y, Y + 1, 1951, (1 << 31) // Z, (1 << 32) // Z, X * Y - 1):
        pts += [k * Z - 1, k * Z, k * Z + 1]
    for k in (1, 2, X // 2, (1 << 31) // (Y * Z), (1 << 31) // (Y * Z) + 1, (1 << 32) // (Y * Z), (1 << 32) // (Y * Z) + 1, X - 1):
        pts += [k * Y * Z - 1, k * Y * Z, k * Y * Z + 1]
    pts = [p for p in pts if 0 <= p < nv]
    return np.concatenate([np.asarray(pts, np.int64), rng.integers(0, nv, 10000, dtype=np.int64)])
