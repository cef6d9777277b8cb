"""Componentwise error bound for the channel-first wavelet level kernels, shared by tests/test_wavelet_paths_gpu.py (the
kernels against the fp64 oracle) and tests/test_wavelet_paths_host.py (which pins this checker on the CPU).

Every element must satisfy   |got - ref64| <= c * 2^-24 * mag   where ref64 is the oracle (oracle/ref_torch.py) run in
float64 on the fp32 inputs and the fp32 filter buffer, and mag is the SAME linear map applied to absolute values: the
sum of |term| over the terms an output is made of, i.e. what a rounding error of one unit in every operation is
relative to.  A max-normalised metric (max|err| / max|ref| over the tensor) cannot see one wrong low-magnitude voxel at
a crop edge or a tile seam; this one compares every voxel with its own scale.

c is derived, in units of 2^-24 (half an fp32 ulp, the bound of one rounding):
  * the separable kernels form a result by three nested fmaf chains of 2K terms each           6K
  * they multiply by the 1-D bank where the oracle multiplies by the fp32 outer-product buffer;
    measured for the project's banks 0.84 / 0.97 / 3.4 / 5.6 units for L = 2 / 4 / 6 / 8
    (ops._factor_bank is bit exact for L = 2 and 4 only)                                        6
  * drop product and the masked rule's (a - b) + b recombination                                3
  * second-order terms                                                                          3
so c = 6K + 12; the dense 4-tap stencil is one 64-term chain without a bank discrepancy: c = 64 + 3.  A factor
gradient is a float-atomic sum over the C channels on top: c + C + 4.
"""
import os

import numpy as np
import torch

from oracle import ref_torch as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

UNIT = 2.0 ** -24
C_DENSE = 64 + 3

# largest last extent the kernels stage in 160 KB of LDS, per filter length: the package's tables, which
# tests/test_wavelet_plans_host.py holds against the plan queries and tests/test_wavelet_paths_host.py against include/lfgc.h
from latent_feature_grid_compression_amd.ops import ADJOINT_MAX_D2, DWT_MAX_N2, SYNTHESIS_MAX_D2  # noqa: E402,F401

# 4 taps, separable: (name, d, t, kernel, ki, zchunk, workgroups along z, len) -- every instantiation of the sliding-window
# kernel at both edges of its range of staged-plane lengths, every remainder of its two-steps-per-trip loop over chunks of
# 5 slices, the tiled kernel at long rows and at the LDS cap, and both sides of the 40 000-voxel switch
DB2_PATHS = [
    ('slide_ki1_one_chunk_of_5', (4, 150, 9), (10, 302, 20), 'sliding_window', 1, 5, 1, 254),
    ('slide_ki1_last_extent_1', (60, 90, 1), (122, 182, 4), 'sliding_window', 1, 5, 13, 132),
    ('slide_ki2_low_edge', (5, 100, 10), (11, 201, 21), 'sliding_window', 2, 5, 2, 262),
    ('slide_ki2_high_edge', (6, 10, 127), (13, 21, 255), 'sliding_window', 2, 5, 2, 510),
    ('slide_ki3_low_edge', (1, 40, 128), (3, 81, 257), 'sliding_window', 3, 2, 1, 514),
    ('slide_ki3_high_edge', (8, 4, 190), (17, 9, 381), 'sliding_window', 3, 5, 2, 762),
    ('tiled_ki4_long_rows', (3, 20, 192), (8, 42, 386), 'tiled_separable', 0, 0, 2, 770),
    ('tiled_at_the_cap', (1, 1, 373), (2, 3, 747), 'tiled_separable', 0, 0, 1, 1121),
    ('threshold_below', (20, 20, 13), (40, 40, 25), 'tiled_separable', 0, 0, 11, 275),
    ('threshold_above', (20, 20, 13), (40, 40, 26), 'sliding_window', 2, 5, 5, 275),
]
DENSE_SHAPES = [((5, 100, 10), (11, 201, 21)), ((6, 10, 127), (13, 21, 255))]
ENCODE_SHAPES = [(3, 5, 757), (2, 2, 2), (7, 300, 3)]


def other_length_shapes(L):
    """L = 2, 6, 8 (tiled separable only): a last extent of 1, a cropped level, the widest row the kernel takes."""
    full = lambda d: tuple(2 * v + L - 2 for v in d)
    cap = (1, 1, SYNTHESIS_MAX_D2[L])
    return [((3, 40, 1), full((3, 40, 1))), ((2, 3, 96), tuple(2 * v + L - 3 for v in (2, 3, 96))), (cap, full(cap))]


def filters(L):
    """(filter_fwd, filter_rev) fp32 CPU: db2 from the oracle's recipe, the others as captured from the reference."""
    if L == 4:
        return R.build_filters(3)
    with np.load(os.path.join(GOLD, 'wavelets_filters.npz')) as z:
        return torch.from_numpy(z['filter_fwd_%d' % L]), torch.from_numpy(z['filter_rev_%d' % L])


def c_separable(K):
    return 6 * K + 12


def c_factor_gradient(c, C):
    return c + C + 4


def worst_ratio(got, ref64, mag):
    """max over ALL elements of |got - ref64| / (2^-24 mag); an element of zero magnitude must be exact (inf otherwise)."""
    got = np.asarray(got, np.float64)
    ref64 = np.asarray(ref64, np.float64)
    mag = np.asarray(mag, np.float64)
    assert got.shape == ref64.shape == mag.shape, (got.shape, ref64.shape, mag.shape)
    assert np.isfinite(got).all() and np.isfinite(ref64).all() and (mag >= 0).all()
    err = np.abs(got - ref64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(mag > 0, err / (UNIT * mag), np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0


def rel_err(y, ref):
    y = np.asarray(y, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    return np.abs(y - ref).max() / max(np.abs(ref).max(), 1e-30)


def oracle_level64(lll, hf, frev64, t):
    """One decode level of the oracle in float64: lll (C,d), hf (C,7,d) -> (C,t)."""
    data = torch.cat([lll.unsqueeze(0).unsqueeze(2), hf.unsqueeze(0)], dim=2)
    return R.wavelet_decode(data, t, frev64)[0]


def _dropped(x, m, thr):
    """The value rules of include/lfgc.h with the gradient of the soft factor."""
    if m is None:
        return x
    if thr is None:
        return x * m.unsqueeze(0)
    return (x * (m >= thr) - x * m).detach() + x * m


def _dropped_mag(x, m, thr):
    if m is None:
        return x
    if thr is None:
        return x * m.unsqueeze(0)
    return x * m.clamp(min=1.0).unsqueeze(0)          # the masked rule handles x, x*m and their difference


def level_reference(lll, hf, frev, t, ml=None, thr_l=None, mh=None, thr_h=None, g=None, pen=None):
    """fp64 reference and magnitudes of one level (fp32 CPU inputs): forward value, and with an upstream gradient g
    (C,t) the gradients of (out * g).sum() + pen . [sum lll^2, sum hf^2, sum |ml|, sum |mh|] (pen: 4 floats or None).
    Returns a dict name -> (ref64, mag) for 'out' and, with g, 'd_lll', 'd_hf', 'd_ml', 'd_mh' (those that exist).
    The gradient magnitudes are the gradients of the same loss built from absolute values (|x|, |m|, |filter|, |g|,
    |pen|): every term enters with its absolute value."""
    dbl = lambda x: None if x is None else x.detach().double()
    f64 = dbl(frev)
    out = {}
    with torch.no_grad():
        fwd_mag = oracle_level64(_dropped_mag(dbl(lll).abs(), None if ml is None else dbl(ml).abs(), thr_l),
                                 _dropped_mag(dbl(hf).abs(), None if mh is None else dbl(mh).abs(), thr_h), f64.abs(), t)
    leaves = {k: dbl(v).requires_grad_(True) for k, v in (('lll', lll), ('hf', hf), ('ml', ml), ('mh', mh)) if v is not None}
    ref = oracle_level64(_dropped(leaves['lll'], leaves.get('ml'), thr_l), _dropped(leaves['hf'], leaves.get('mh'), thr_h), f64, t)
    out['out'] = (ref.detach().numpy(), fwd_mag.numpy())
    if g is None:
        return out
    ab = {k: dbl(v).abs().requires_grad_(True) for k, v in (('lll', lll), ('hf', hf), ('ml', ml), ('mh', mh)) if v is not None}
    loss = (ref * dbl(g)).sum()
    loss_abs = (oracle_level64(_dropped(ab['lll'], ab.get('ml'), None), _dropped(ab['hf'], ab.get('mh'), None), f64.abs(), t)
                * dbl(g).abs()).sum()
    if pen is not None:
        terms = lambda s: [(s['lll'] ** 2).sum(), (s['hf'] ** 2).sum(),
                           s['ml'].abs().sum() if 'ml' in s else 0.0, s['mh'].abs().sum() if 'mh' in s else 0.0]
        loss = loss + sum(float(w) * v for w, v in zip(pen, terms(leaves)))
        loss_abs = loss_abs + sum(abs(float(w)) * v for w, v in zip(pen, terms(ab)))
    loss.backward()
    loss_abs.backward()
    for k in leaves:
        out['d_' + k] = (leaves[k].grad.numpy(), ab[k].grad.numpy())
    return out


def encode_reference(x, ffwd):
    """fp64 reference and magnitude of one forward-DWT level: x (C,n) fp32 -> (C,8,d)."""
    with torch.no_grad():
        ref, _ = R.wavelet_encode(x.double().unsqueeze(0), ffwd.double())
        mag, _ = R.wavelet_encode(x.double().abs().unsqueeze(0), ffwd.double().abs())
    return ref[0].numpy(), mag[0].numpy()


# ---- numpy fp32 restatement of the separable synthesis (csrc/lfgc_wavelet.hip: idwt_level_kernel, SEP build) -------------

def _fma(a, b, t):
    """fmaf on fp32 arrays: the product of two fp32 is exact in fp64; the sum is rounded to fp64, then to fp32."""
    return (a.astype(np.float64) * np.float64(b) + t.astype(np.float64)).astype(np.float32)


def _contract(lo, hi, bank, K, leak=None, tap_shift=False):
    """One axis (the last of lo / hi) of the synthesis: out[2 jj + p] = chain over e, s of in_s[jj - e] * bank[s][p + 2 e],
    jj in [0, d + K - 1), in the kernel's order (neighbour e outer, band s inner), cells outside [0, d) reading zero.
    leak: an array of lo's shape without the last axis, read at cell index d instead of zero -- (lo_leak, hi_leak).
    tap_shift: the high band's first tap of parity 0 is read one index too far (Haar's two low taps are equal)."""
    d = lo.shape[-1]
    n = d + K - 1
    pad = [(0, 0)] * (lo.ndim - 1) + [(K - 1, K - 1)]
    P = [np.pad(lo, pad), np.pad(hi, pad)]
    if leak is not None and K > 1:
        for s in range(2):
            P[s][..., K - 1 + d] = leak[s]
    out = np.zeros(lo.shape[:-1] + (2 * n,), np.float32)
    for p in range(2):
        t = np.zeros(lo.shape[:-1] + (n,), np.float32)
        for e in range(K):
            for s in range(2):
                tap = p + 2 * e + (1 if (tap_shift and p == 0 and e == 0 and s == 1) else 0)
                t = _fma(P[s][..., K - 1 - e:K - 1 - e + n], bank[s][tap], t)
        out[..., p::2] = t
    return out


def separable_level_fp32(lll, hf, bank, t, bug=None):
    """The kernel's arithmetic in numpy fp32: contract x, then y, then z with 2K-term fmaf chains, then crop to t.
    lll (C,d0,d1,d2), hf (C,7,d0,d1,d2) fp32, bank (2,L) fp32 (ops._factor_bank).
    bug = 'select': the x-range select of the neighbour at x = d2 is dropped, so that cell reads what lies behind it in
    the staged plane -- the next row's first cell (zeros behind the last row); 'tap': one tap index shifted by one."""
    bank = np.asarray(bank, np.float32)
    K = bank.shape[1] // 2
    C = lll.shape[0]
    bands = np.concatenate([lll[:, None], hf], axis=1).astype(np.float32)      # (C, 8, d0,d1,d2), band = 4 sz + 2 sy + sx
    b = bands.reshape((C, 2, 2, 2) + bands.shape[2:])                          # [sz][sy][sx]
    leak = None
    if bug == 'select':
        nxt = np.zeros(b.shape[:-1], np.float32)                               # [..., z, y]: cell (y + 1, x = 0)
        nxt[..., :-1] = b[..., 1:, 0]
        leak = (nxt[:, :, :, 0], nxt[:, :, :, 1])
    X = _contract(b[:, :, :, 0], b[:, :, :, 1], bank, K, leak=leak, tap_shift=(bug == 'tap'))   # (C, sz, sy, z, y, X)
    X = np.moveaxis(X, -2, -1)                                                 # (C, sz, sy, z, X, y)
    Y = _contract(X[:, :, 0], X[:, :, 1], bank, K)                             # (C, sz, z, X, Y)
    Y = np.moveaxis(Y, -3, -1)                                                 # (C, sz, X, Y, z)
    Z = _contract(Y[:, 0], Y[:, 1], bank, K)                                   # (C, X, Y, Z)
    full = np.transpose(Z, (0, 3, 2, 1))                                       # (C, Z, Y, X)
    off = [(full.shape[1 + a] - t[a]) // 2 for a in range(3)]
    return np.ascontiguousarray(full[:, off[0]:off[0] + t[0], off[1]:off[1] + t[1], off[2]:off[2] + t[2]])
