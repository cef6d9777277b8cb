"""GPU tests of every launch path of the channel-first wavelet level kernels (csrc/lfgc_wavelet.hip) against the oracle
run in float64, under a componentwise bound (tests/wavelet_bound.py: |got - ref64| <= c * 2^-24 * mag for EVERY element,
mag = the same linear map on absolute values, c derived from the length of the kernels' fmaf chains) with the
max-normalised bounds of tests/test_wavelets_gpu.py kept beside it.  Each case first asks the library which kernel its
shape reaches (ops.idwt_level_plan and relatives: the launcher consumes the struct the query fills), so a change of the
selection that would leave a path untested fails here, and tests/test_wavelet_plans_host.py holds the same table on the CPU.

Paths: the three instantiations of the sliding-window kernel at both edges of their ranges with every remainder of its
chunk loop, plain and with the drop factors (plain and masked rule), the penalty fold and the deterministic slice mode of
the adjoint; the tiled separable kernel at long rows (more than 64 KB of LDS) and at the LDS cap for all four filter
lengths, with the refusal just past it; the dense 4-tap stencil above the small-level switch; the forward DWT at long and
degenerate rows; the layout conversion, second channel pass included, bit for bit.

Worst measured ratios err / (2^-24 mag) per path are recorded in DESIGN.md (wavelet section); every case prints its own."""
import ctypes
import os

import numpy as np
import pytest
import torch

import wavelet_bound as W

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -3
SENTINEL = -12345.5
SLIDE = {c[0]: c for c in W.DB2_PATHS}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))      # the fp64 oracle runs on the CPU
    return torch.device('cuda:0')


def rel_err(y, ref):
    return W.rel_err(y, ref)


def _rand(rng, *shape):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32))


def _unif(rng, *shape):
    return torch.from_numpy(rng.uniform(-1.0, 1.0, shape).astype(np.float32))


def check(tag, name, got, ref, mag, c, max_bound):
    """Both bounds on one tensor; prints the worst componentwise ratio."""
    got = got.detach().cpu().numpy()
    ratio = W.worst_ratio(got, ref, mag)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print('%s %s: worst %.2f units of 2^-24 mag (bound %d), max|err| %.3g' % (tag, name, ratio, c, err))
    assert ratio <= c, (tag, name, ratio, c)
    assert err <= max_bound, (tag, name, err, max_bound)


def run_level(dev, tag, L, C, d, t, ml=None, thr_l=None, mh=None, thr_h=None, pen=None, deterministic=False, seed=0):
    """Forward and adjoint of one level through the ops wrappers against the fp64 oracle.  ml / mh: 'u' draws uniform
    [-1, 1] factors.  pen: 4 upstream penalty gradients (0 = none) folded into the adjoint."""
    from latent_feature_grid_compression_amd import ops
    K = L // 2
    c = W.c_separable(K)
    _, frev = W.filters(L)
    rng = np.random.default_rng(1000 * L + 10 * C + seed)
    lll, hf, g = _rand(rng, C, *d), _rand(rng, C, 7, *d), _rand(rng, C, *t)
    ml = _unif(rng, *d) if ml is not None else None
    mh = _unif(rng, 7, *d) if mh is not None else None
    drop = ml is not None or mh is not None
    r = W.level_reference(lll, hf, frev, t, ml, thr_l, mh, thr_h, g, pen)
    to = lambda x: None if x is None else x.to(dev)
    frev_d = frev.to(dev)
    if drop:
        got = ops.idwt_level_drop(to(lll), to(hf), to(ml), thr_l, to(mh), thr_h, frev_d, t)
    else:
        got = ops.idwt_level(to(lll), to(hf), frev_d, t)
    ref, mag = r['out']
    check(tag, 'out', got, ref, mag, c, 1e-6 * max(float(np.abs(ref).max()), 1e-30))
    if drop or pen is not None:
        ptrs, keep = None, None
        if pen is not None:
            keep = torch.tensor(pen, dtype=torch.float32, device=dev)
            ptrs = [keep[i:i + 1].data_ptr() if pen[i] != 0 else 0 for i in range(4)]
        if deterministic:
            grads = ops._adjoint(to(g), None, frev_d, to(lll), to(hf), to(ml), to(mh), ml is not None, mh is not None, d,
                                 ptrs, False, deterministic=True)
        else:
            grads = ops.idwt_level_drop_bwd(to(g), frev_d, to(lll), to(hf), to(ml), to(mh), ml is not None, mh is not None,
                                            d, ptrs)
        torch.cuda.synchronize()
    else:
        grads = ops.idwt_level_bwd(to(g), frev_d, d) + (None, None)
    for name, got, cc in (('d_lll', grads[0], c), ('d_hf', grads[1], c), ('d_ml', grads[2], W.c_factor_gradient(c, C)),
                          ('d_mh', grads[3], W.c_factor_gradient(c, C))):
        if name in r:
            assert got is not None, name
            ref, mag = r[name]
            check(tag, name, got, ref, mag, cc, 5e-6 * max(1.0, float(np.abs(ref).max())))
        else:
            assert got is None, name


def assert_plan(L, C, d, t, kernel, ki=0, zchunk=0, gy=None, drop=False, has_taps=True):
    from latent_feature_grid_compression_amd import ops
    p = ops.idwt_level_plan(L, C, d, t, has_taps=has_taps, has_drop=drop)
    assert (p.kernel, p.ki, p.zchunk, p.drop) == (kernel, ki, zchunk, drop), p
    if gy is not None:
        assert p.grid[1] == gy, p
    b = ops.idwt_level_bwd_plan(L, C, d, t, has_taps=has_taps, has_drop=drop)
    assert b.kernel == ('analysis_separable' if has_taps else 'analysis_dense') and b.drop == drop, b
    return p


# ---- 4 taps, separable ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,d,t,kernel,ki,zchunk,gy,length', W.DB2_PATHS, ids=[c[0] for c in W.DB2_PATHS])
def test_db2_paths(dev, name, d, t, kernel, ki, zchunk, gy, length):
    C = 3 if name.startswith('threshold') else 2
    p = assert_plan(4, C, d, t, kernel, ki, zchunk, gy)
    assert p.len == length
    run_level(dev, name, 4, C, d, t)


@pytest.mark.parametrize('variant', ['plain_both', 'masked_detail'])
@pytest.mark.parametrize('name,d,t,kernel,ki,zchunk,gy,length', W.DB2_PATHS[:7], ids=[c[0] for c in W.DB2_PATHS[:7]])
def test_db2_paths_with_drop_factors(dev, name, d, t, kernel, ki, zchunk, gy, length, variant):
    C = 3
    assert_plan(4, C, d, t, kernel, ki, zchunk, gy, drop=True)
    if variant == 'plain_both':
        run_level(dev, name + ' ' + variant, 4, C, d, t, ml='u', mh='u', seed=1)
    else:
        run_level(dev, name + ' ' + variant, 4, C, d, t, mh='u', thr_h=0.5, seed=2)


def test_slide_row_with_penalty_fold(dev):
    """The L2 penalty of both coefficient tensors and the L1 penalty of both factors folded into the adjoint."""
    name, d, t, kernel, ki, zchunk, gy, _ = SLIDE['slide_ki2_low_edge']
    assert_plan(4, 3, d, t, kernel, ki, zchunk, gy, drop=True)
    run_level(dev, name + ' penalties', 4, 3, d, t, ml='u', mh='u', pen=[0.7, -1.3, 0.4, 2.1], seed=3)
    # an L2 penalty alone (no factors) takes the DROP build of the adjoint as well
    run_level(dev, name + ' l2 only', 4, 3, d, t, pen=[0.7, -1.3, 0.0, 0.0], seed=4)


def test_slide_row_deterministic_slices(dev):
    """The deterministic mode of the factor gradients (one slice per channel, folded in channel order): same bound."""
    name, d, t, kernel, ki, zchunk, gy, _ = SLIDE['slide_ki3_high_edge']
    assert_plan(4, 3, d, t, kernel, ki, zchunk, gy, drop=True)
    run_level(dev, name + ' deterministic', 4, 3, d, t, ml='u', mh='u', pen=[0.0, 0.5, 0.0, -0.8], deterministic=True, seed=5)


def test_4tap_refusal_past_the_cap(dev):
    _refusal(dev, 4)


# ---- 4 taps, dense -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('d,t', W.DENSE_SHAPES)
def test_dense_stencil_above_the_small_level_switch(dev, d, t):
    """taps = NULL with the db2 buffer: one 64-term chain per output, the bank discrepancy does not apply."""
    from latent_feature_grid_compression_amd import ops, _lib
    lib = _lib.load()
    C = 2
    p = assert_plan(4, C, d, t, 'tiled_dense', has_taps=False)
    assert p.grid[1] == (d[0] + 2) // 2
    _, frev = W.filters(4)
    rng = np.random.default_rng(400 + d[0])
    lll, hf, g = _rand(rng, C, *d), _rand(rng, C, 7, *d), _rand(rng, C, *t)
    r = W.level_reference(lll, hf, frev, t, g=g)
    frev_d, lll_d, hf_d, g_d = (x.to(dev).contiguous() for x in (frev, lll, hf, g))
    out = torch.full((C,) + t, SENTINEL, device=dev)
    d_l, d_h = torch.full((C,) + d, SENTINEL, device=dev), torch.full((C, 7) + d, SENTINEL, device=dev)
    s = ops._stream(lll_d)
    assert lib.lfgc_idwt_level_f32(lll_d.data_ptr(), hf_d.data_ptr(), frev_d.data_ptr(), None, out.data_ptr(), C, *d, *t, s) == 0
    assert lib.lfgc_idwt_level_bwd_f32(g_d.data_ptr(), frev_d.data_ptr(), None, d_l.data_ptr(), d_h.data_ptr(), C, *d, *t, s) == 0
    torch.cuda.synchronize()
    tag = 'dense %s' % (d,)
    ref, mag = r['out']
    check(tag, 'out', out, ref, mag, W.C_DENSE, 1e-6 * float(np.abs(ref).max()))
    for name, got in (('d_lll', d_l), ('d_hf', d_h)):
        ref, mag = r[name]
        check(tag, name, got, ref, mag, W.C_DENSE, 5e-6 * max(1.0, float(np.abs(ref).max())))


# ---- L = 2, 6, 8 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L', [2, 6, 8])
@pytest.mark.parametrize('which', [0, 1, 2], ids=['last_extent_1', 'cropped', 'cap'])
def test_other_lengths(dev, L, which):
    d, t = W.other_length_shapes(L)[which]
    K = L // 2
    for drop in (False, True):
        p = assert_plan(L, 2, d, t, 'tiled_separable', gy=(d[0] + K) // 2, drop=drop)
        assert p.lds_bytes <= 160 * 1024
    tag = 'L=%d %s' % (L, d)
    run_level(dev, tag, L, 2, d, t)
    if which == 1:
        run_level(dev, tag + ' plain_both', L, 2, d, t, ml='u', mh='u', seed=1)
    else:
        run_level(dev, tag + ' masked_detail', L, 2, d, t, mh='u', thr_h=0.5, seed=2)


def _refusal(dev, L):
    """One past the widest row: refused on the host by the synthesis and its drop variant, nothing launched (the output
    keeps its sentinel), and the wrapper names the limit."""
    from latent_feature_grid_compression_amd import ops, _lib
    lib = _lib.load()
    lim = W.SYNTHESIS_MAX_D2[L]
    C, d = 2, (1, 1, lim + 1)
    t = tuple(2 * v + L - 2 for v in d)
    _, frev = W.filters(L)
    frev_d = frev.to(dev)
    taps = ops.filter_taps(frev_d)
    assert taps is not None
    info = _lib.WaveletPlanInfo()
    assert lib.lfgc_idwt_level_plan(L, 1, 0, C, *d, *t, ctypes.byref(info)) == E_UNSUPPORTED
    lll, hf = torch.ones((C,) + d, device=dev), torch.ones((C, 7) + d, device=dev)
    mh = torch.ones((7,) + d, device=dev)
    out = torch.full((C,) + t, SENTINEL, device=dev)
    s = ops._stream(lll)
    nan = float('nan')
    assert lib.lfgc_idwt_level_len_f32(lll.data_ptr(), hf.data_ptr(), frev_d.data_ptr(), taps, L, out.data_ptr(), C, *d, *t, s) == E_UNSUPPORTED
    assert lib.lfgc_idwt_level_drop_len_f32(lll.data_ptr(), hf.data_ptr(), None, nan, mh.data_ptr(), 0.5, frev_d.data_ptr(), taps,
                                            L, out.data_ptr(), C, *d, *t, s) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(NotImplementedError, match='at most %d for %d taps in the synthesis' % (lim, L)):
        ops.idwt_level(lll, hf, frev_d, t)
    with pytest.raises(NotImplementedError, match='at most %d for %d taps in the synthesis' % (lim, L)):
        ops.idwt_level_drop(lll, hf, None, None, mh, 0.5, frev_d, t)
    # the adjoint stages rows of the gradient and still takes this level
    d_l, d_h = ops.idwt_level_bwd(torch.ones((C,) + t, device=dev), frev_d, d)
    assert d_l.shape == (C,) + d and bool(torch.isfinite(d_h).all())


@pytest.mark.parametrize('L', [2, 6, 8])
def test_other_lengths_refusal_past_the_cap(dev, L):
    _refusal(dev, L)


# ---- forward DWT ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('L', [2, 4, 6, 8])
def test_encode(dev, L):
    """Long rows, the smallest input and a last extent of 3.  (3,5,757) is the output row of the widest 4-tap level; the
    6- and 8-tap encodes take rows up to 638 and 408 (include/lfgc.h) and refuse it on the host -- there the widest row
    of their own synthesis limit runs instead, and the refusal is checked."""
    from latent_feature_grid_compression_amd import ops, _lib
    lib = _lib.load()
    ffwd, _ = W.filters(L)
    ffwd_d = ffwd.to(dev)
    c = W.c_separable(L // 2)
    for n in W.ENCODE_SHAPES + [(3, 5, 2 * W.SYNTHESIS_MAX_D2[L] + L - 2)]:
        rng = np.random.default_rng(L * 100 + n[2])
        x = _rand(rng, 3, *n)
        if n[2] > W.DWT_MAX_N2[L]:
            assert L in (6, 8) and n == (3, 5, 757)
            dshape = ops.dwt_out_shape(n, L)
            out = torch.full((3, 8) + tuple(dshape), SENTINEL, device=dev)
            x_d = x.to(dev)
            assert lib.lfgc_dwt_level_len_f32(x_d.data_ptr(), ffwd_d.data_ptr(), ops.filter_taps(ffwd_d), L, out.data_ptr(),
                                              3, *n, ops._stream(x_d)) == E_UNSUPPORTED
            torch.cuda.synchronize()
            assert bool((out == SENTINEL).all())
            with pytest.raises(NotImplementedError, match='at most %d for %d taps' % (W.DWT_MAX_N2[L], L)):
                ops.dwt_level(x_d, ffwd_d)
            continue
        assert ops.dwt_level_plan(L, 3, n).kernel == 'analysis_separable'
        ref, mag = W.encode_reference(x, ffwd)
        got = ops.dwt_level(x.to(dev), ffwd_d)
        assert tuple(got.shape) == ref.shape, (L, n)
        check('encode L=%d %s' % (L, n), 'out', got, ref, mag, c, 1e-6 * float(np.abs(ref).max()))


# ---- layout --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [1, 8, 31, 32, 33, 40, 64, 65])
def test_layout_conversion_is_exact(dev, C):
    """permute + zero pad, bit for bit, through one and several passes of the kernels' 32-channel loop and through partial
    64-voxel tiles; the round trip returns the input."""
    from latent_feature_grid_compression_amd import ops
    cs = ops.grid_channel_stride(C)
    assert cs >= C and cs % 8 == 0 and cs - C < 8
    for V in (1, 63, 64, 65, 4097):
        rng = np.random.default_rng(C * 10000 + V)
        x = _rand(rng, C, 1, 1, V).to(dev)
        want = torch.zeros((1, 1, V, cs), device=dev)
        want[..., :C] = x.permute(1, 2, 3, 0)
        got = ops.to_channel_last(x)
        assert got.shape == want.shape and torch.equal(got, want), (C, V)
        if cs > C:
            assert float(got[..., C:].abs().max()) == 0.0
        back = ops.to_channel_first(got, C)
        assert back.shape == x.shape and torch.equal(back, x), (C, V)
        # pad channels of the source are ignored on the way back
        noisy = got.clone()
        noisy[..., C:] = 7.0
        assert torch.equal(ops.to_channel_first(noisy, C), x), (C, V)
