"""Componentwise error bound for the wavelet level kernels, shared by tests/test_wavelet_paths_gpu.py and
tests/test_wavelet_cl_paths_gpu.py (the channel-first and the channel-last kernels against the fp64 oracle) and by
tests/test_wavelet_paths_host.py and tests/test_wavelet_cl_plans_host.py (which pin this checker on the CPU).

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


def _contract(lo, hi, bank, K, leak=None, tap_shift=False, seam=0):
    """One axis (the last of lo / hi) of the synthesis: out[2 jj + p] = chain over e, s of in_s[jj - e] * bank[s][p + 2 e],
    jj in [0, d + K - 1), in the kernel's order (neighbour e outer, band s inner), cells outside [0, d) reading zero.
    leak: an array of lo's shape without the last axis, read at cell index d instead of zero -- (lo_leak, hi_leak).
    tap_shift: the high band's first tap of parity 0 is read one index too far (Haar's two low taps are equal).
    seam: chunks of `seam` cells that start without their warm-up cells -- cell jj of a chunk beginning at b > 0 loses the
    terms of the cells jj - e < b."""
    d = lo.shape[-1]
    n = d + K - 1
    pad = [(0, 0)] * (lo.ndim - 1) + [(K - 1, K - 1)]
    P = [np.pad(lo, pad), np.pad(hi, pad)]
    if leak is not None and K > 1:
        for s in range(2):
            P[s][..., K - 1 + d] = leak[s]
    jj = np.arange(n)
    begin = (jj // seam) * seam if seam else np.zeros(n, np.int64)
    out = np.zeros(lo.shape[:-1] + (2 * n,), np.float32)
    for p in range(2):
        t = np.zeros(lo.shape[:-1] + (n,), np.float32)
        for e in range(K):
            keep = ((jj - e >= begin) | (begin == 0)).astype(np.float32)     # all ones without a seam
            for s in range(2):
                tap = p + 2 * e + (1 if (tap_shift and p == 0 and e == 0 and s == 1) else 0)
                t = _fma(P[s][..., K - 1 - e:K - 1 - e + n] * keep, bank[s][tap], t)
        out[..., p::2] = t
    return out


def separable_level_fp32(lll, hf, bank, t, bug=None, zchunk=0):
    """The kernel's arithmetic in numpy fp32: contract x, then y, then z with 2K-term fmaf chains, then crop to t.
    lll (C,d0,d1,d2), hf (C,7,d0,d1,d2) fp32, bank (2,L) fp32 (ops._factor_bank).
    bug = 'select': the x-range select of the neighbour at x = d2 is dropped, so that cell reads what lies behind it in
    the staged plane -- the next row's first cell (zeros behind the last row); 'tap': one tap index shifted by one;
    'seam': the z walk of the channel-last kernels (csrc/lfgc_wavelet_cl.hip) in chunks of `zchunk` cell slices, each
    chunk after the first starting WITHOUT its warm-up planes: the cell slices jz_begin .. jz_begin + K - 2 lose what the
    coefficient planes jz_begin - 1 .. jz_begin - (K - 1) carry into them."""
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
    Z = _contract(Y[:, 0], Y[:, 1], bank, K, seam=(zchunk if bug == 'seam' else 0))   # (C, X, Y, Z)
    full = np.transpose(Z, (0, 3, 2, 1))                                       # (C, Z, Y, X)
    off = [(full.shape[1 + a] - t[a]) // 2 for a in range(3)]
    return np.ascontiguousarray(full[:, off[0]:off[0] + t[0], off[1]:off[1] + t[1], off[2]:off[2] + t[2]])


# ---- channel-last last level (csrc/lfgc_wavelet_cl.hip): the launch rules restated, the cases, their references ----------
# Shared by tests/test_wavelet_cl_plans_host.py (the plan queries against these rules, no device) and
# tests/test_wavelet_cl_paths_gpu.py (every case asserts its plan, then runs it against level_reference).

CL_CELLS = 32
CL_LDS_CAP = 80 * 1024
CL_KNOBS = {'cw': 'LFGC_CL_CW', 'nt': 'LFGC_CL_NT', 'ng': 'LFGC_CL_ADJ_NG', 'nchunks': 'LFGC_CL_NCHUNKS'}


def _ceil(a, b):
    return -(-a // b)


def cl_pick_zchunk(columns, nz, slots_per_cu, num_cus, nchunks=None):
    """z steps per work item.  The rule as the source states it: few enough workgroups per slot that no round is mostly
    idle, long enough that the warm-up plane of a chunk stays a small share -- the chunk count in 1..nz whose
    rounds * (zchunk + 1) is smallest, the first one on a tie; a forced count in 1..nz wins, any other is ignored."""
    if nchunks is not None and 1 <= nchunks <= nz:
        return _ceil(nz, nchunks)
    slots = slots_per_cu * num_cus
    best_cost, best = None, nz
    for n in range(1, nz + 1):
        zc = _ceil(nz, n)
        cost = _ceil(columns * _ceil(nz, zc), slots) * (zc + 1)
        if best_cost is None or cost < best_cost:
            best_cost, best = cost, zc
    return best


def cl_expected_plan(adjoint, L, C, d, t, drop, num_cus, cw=None, nt=None, ng=None, nchunks=None):
    """The launch of the channel-last level as the source comments and DESIGN section 3.2.1 give it; cw / nt / ng / nchunks:
    the diagnostics knobs' values (None: not set).  Returns a dict of the fields of lfgc_wavelet_cl_plan_info."""
    K = L // 2
    cs = _ceil(C, 8) * 8
    if not adjoint:
        ptiles = _ceil((d[1] + K - 1) * (d[2] + K - 1), CL_CELLS)
        w = (32 if ptiles >= 96 else 16) if cs == 32 else 16 if cs == 16 else 8
        if cw in (8, 16, 32) and cs % cw == 0:
            w = cw
        cells = CL_CELLS
        lds = 2 * 8 * CL_CELLS * (w + 1) * 4 + (2 * 8 * K * K * CL_CELLS * 4 if drop else 0)
        stream = w == 32 and t[0] * t[1] * t[2] * cs * 4 > 48 << 20
        if nt is not None:
            stream = str(nt)[0] == '1'
        slots = {32: 1, 16: 2, 8: 4}[w]
        nz = d[0] + K - 1
    else:
        w = 16 if cs % 16 == 0 else 8
        g = 2 if d[1] * d[2] >= 3072 else 1
        if ng in (1, 2):
            g = ng
        cells = CL_CELLS * g
        ptiles = _ceil(d[1] * d[2], cells)
        lds = 2 * w * (8 * cells + 1) * 4
        stream = False
        slots = (2 if g == 2 else 3) if w == 16 else (4 if g == 2 else 6)
        if drop and K == 2 and g == 1:
            slots = 2 if w == 16 else 5
        nz = d[0]
    ngroups = cs // w
    zchunk = cl_pick_zchunk(ptiles * ngroups, nz, slots, num_cus, nchunks)
    n = _ceil(nz, zchunk)
    return dict(cw=w, cells=cells, nt=stream, drop=bool(drop), zchunk=zchunk, nchunks=n, ptiles=ptiles, ngroups=ngroups,
                threads=32 * w, lds_bytes=lds, blocks=_ceil(ptiles * ngroups * n, 8) * 8)


def cl_target(L, d):
    """Targets of the channel-last cases: db2 cropped by one on one axis (which one rotates with the shape), Haar
    min(that, 2 d) = its full level."""
    t = [2 * v + 2 for v in d]
    t[sum(d) % 3] -= 1
    return tuple(t) if L == 4 else tuple(min(tv, 2 * dv) for tv, dv in zip(t, d))


# (name, C, d, knobs, synthesis CW, adjoint CW, adjoint cell groups NG): the smallest shapes that reach each path
CL_ROWS = [
    ('cw32_ng2', 32, (2, 56, 56), {}, 32, 16, 2),              # ptiles 102 (db2) / 98 (Haar); d1 d2 = 3136 >= 3072
    ('cw16_stride32', 30, (5, 9, 12), {}, 16, 16, 1),
    ('cw16_stride16', 13, (5, 12, 7), {}, 16, 16, 1),
    ('cw8_one_group', 5, (6, 7, 9), {}, 8, 8, 1),
    ('cw8_three_groups', 22, (4, 35, 6), {}, 8, 8, 1),
    ('cw8_forced_stride32', 30, (5, 9, 12), {'cw': 8}, 8, 16, 1),
    ('cw32_forced_small_plane', 30, (5, 9, 12), {'cw': 32}, 32, 16, 1),
    ('one_cell_one_plane', 3, (1, 1, 1), {}, 8, 8, 1),
    ('adj_cw8_ng2', 8, (2, 56, 56), {}, 8, 8, 2),
    ('adj_ng2_forced_ragged_cw16', 30, (5, 9, 12), {'ng': 2}, 16, 16, 2),      # 108 cells: second group of tile 2 ragged
    ('adj_ng2_forced_ragged_cw8', 5, (5, 9, 12), {'ng': 2}, 8, 8, 2),
    ('adj_ng2_forced_empty_group', 13, (3, 7, 10), {'ng': 2}, 16, 16, 2),      # 70 cells: tile 2's second group empty
]
CL_ROW = {r[0]: r for r in CL_ROWS}
CL_MASKED_ROWS = ('cw32_ng2', 'cw16_stride32', 'cw16_stride16', 'adj_ng2_forced_ragged_cw16', 'adj_ng2_forced_empty_group')
CL_PENALTY = [0.7, -1.3, 0.4, 2.1]
CL_WIDE = [(40, (5, 6, 7)), (48, (5, 6, 7))]       # C > 32 through the plain pair's C ABI
# z chunks: nz = 7 steps forced into 1, 2, 3 and 7 chunks of 7 / 4+3 / 3+3+1 / 1 each
CL_NCHUNKS = (1, 2, 3, 7)
CL_CHUNK_ROWS = [('cw16_stride16', 13, (12, 7)), ('cw8_one_group', 5, (7, 9))]


def cl_chunk_shape(L, plane, adjoint):
    """d with 7 z steps: the synthesis walks d0 + K - 1 cell slices, the adjoint d0 planes."""
    return ((7 if adjoint else 8 - L // 2),) + tuple(plane)


_CL_REFS = {}


def cl_case(L, C, d, variant='plain', pen=None, adjoint=True):
    """Inputs and fp64 reference of one channel-last case, computed once per process: standard-normal coefficients and
    gradient, factors uniform in [-1, 1].  variant: 'plain', 'drop' (both factors, product rule), 'masked' (both factors,
    threshold 0.5).  Returns a SimpleNamespace: lll, hf, g, ml, mh, thr, t, ref (name -> (ref64, mag)).  Every magnitude
    is asserted positive: no element of any tensor is outside the componentwise bound."""
    from types import SimpleNamespace
    key = (L, C, tuple(d), variant, None if pen is None else tuple(pen), adjoint)
    if key in _CL_REFS:
        return _CL_REFS[key]
    t = cl_target(L, d)
    _, frev = filters(L)
    rng = np.random.default_rng([L, C, *d, ('plain', 'drop', 'masked').index(variant)])
    f = lambda draw, *s: torch.from_numpy(draw(s).astype(np.float32))
    normal, unif = rng.standard_normal, (lambda s: rng.uniform(-1.0, 1.0, s))
    lll, hf, g = f(normal, C, *d), f(normal, C, 7, *d), f(normal, C, *t)
    ml = mh = thr = None
    if variant != 'plain':
        ml, mh = f(unif, *d), f(unif, 7, *d)
        thr = 0.5 if variant == 'masked' else None
    ref = level_reference(lll, hf, frev, t, ml, thr, mh, thr, g if adjoint else None, pen)
    for name, (r, mag) in ref.items():
        assert (mag > 0).all(), (key, name)
    case = SimpleNamespace(L=L, C=C, d=tuple(d), t=t, frev=frev, lll=lll, hf=hf, g=g, ml=ml, mh=mh, thr=thr, pen=pen, ref=ref)
    _CL_REFS[key] = case
    return case
