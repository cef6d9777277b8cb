"""CPU test of the componentwise checker tests/test_wavelet_paths_gpu.py judges the kernels with (tests/wavelet_bound.py):
a numpy fp32 restatement of the separable synthesis -- the kernel's contraction order, x then y then z in 2K-term fmaf
chains with the bank of ops._factor_bank -- passes the bound against the fp64 oracle, the same restatement with one
boundary select dropped or one tap index shifted does not, and a max-normalised metric alone would let the dropped select
through once the voxels it touches are small against the rest of the tensor.

Measured here (d = (3,4,9), cropped, K = 1..4): the restatement lands at 2.1 to 2.6 units of 2^-24 * mag against bounds of
18 to 36; the dropped select and the shifted tap at 1e5 to 1e7 units.  The dropped select's error is 0.30 to 0.49 of the
tensor's largest value when the voxels it touches are as large as the rest, so max|err| / max|ref| <= 1e-6 still sees it
with those voxels scaled to 1e-4 of the rest (3.1e-5 to 4.9e-5 measured) and loses it below about 2e-6; the assertion
that the max-normalised metric misses it is therefore made at 1e-7, and at 1e-4 the test asserts that it does not."""
import numpy as np
import pytest
import torch

import wavelet_bound as W

D = (3, 4, 9)
CROP = (1, 2, 1)


def _case(K, seed=0):
    from latent_feature_grid_compression_amd import ops
    L = 2 * K
    _, frev = W.filters(L)
    bank = ops._factor_bank(frev.numpy())
    assert bank is not None and bank.shape == (2, L)
    t = tuple(2 * v + L - 2 - c for v, c in zip(D, CROP))
    rng = np.random.default_rng(100 * K + seed)
    lll = rng.standard_normal((2,) + D).astype(np.float32)
    hf = rng.standard_normal((2, 7) + D).astype(np.float32)
    return frev, bank, t, lll, hf


def _reference(lll, hf, frev, t):
    return W.level_reference(torch.from_numpy(lll), torch.from_numpy(hf), frev, t)['out']


@pytest.mark.parametrize('K', [1, 2, 3, 4])
def test_restatement_passes_and_seeded_bugs_fail(K):
    frev, bank, t, lll, hf = _case(K)
    ref, mag = _reference(lll, hf, frev, t)
    good = W.separable_level_fp32(lll, hf, bank, t)
    assert good.shape == ref.shape
    ratio = W.worst_ratio(good, ref, mag)
    print('K=%d restatement: %.2f units (bound %d), max-normalised %.2e' % (K, ratio, W.c_separable(K), W.rel_err(good, ref)))
    assert ratio <= W.c_separable(K)
    assert W.rel_err(good, ref) <= 1e-6
    shifted = W.separable_level_fp32(lll, hf, bank, t, bug='tap')
    assert W.worst_ratio(shifted, ref, mag) > W.c_separable(K)
    leaky = W.separable_level_fp32(lll, hf, bank, t, bug='select')
    if K == 1:
        # Haar has no neighbour cells and no x-range select (x_in_level is constant true for K = 1)
        assert np.array_equal(leaky, good)
    else:
        assert W.worst_ratio(leaky, ref, mag) > W.c_separable(K)


@pytest.mark.parametrize('K', [2, 3, 4])
def test_max_normalised_metric_misses_a_dropped_select_on_small_voxels(K):
    """Why the bound is componentwise.  The dropped select adds the next row's first cell to the outputs of the cell column
    x = d2.  With the coefficients those outputs are made of (the last K - 1 columns, which are all their legitimate
    neighbours) and the leaked column x = 0 scaled to s of the rest, error and magnitude of the touched voxels scale by s
    alike: the componentwise ratio does not move, max|err| / max|ref| shrinks by s."""
    frev, bank, t, lll, hf = _case(K)
    d2 = D[2]
    for s, hidden in ((1.0, False), (1e-4, False), (1e-7, True)):
        l2, h2 = lll.copy(), hf.copy()
        for x in (l2, h2):
            x[..., 0] *= np.float32(s)
            x[..., d2 - (K - 1):] *= np.float32(s)
        ref, mag = _reference(l2, h2, frev, t)
        good = W.separable_level_fp32(l2, h2, bank, t)
        leaky = W.separable_level_fp32(l2, h2, bank, t, bug='select')
        print('K=%d s=%g: dropped select %.3g units, max-normalised %.3g (clean: %.2f units, %.3g)'
              % (K, s, W.worst_ratio(leaky, ref, mag), W.rel_err(leaky, ref), W.worst_ratio(good, ref, mag), W.rel_err(good, ref)))
        assert W.worst_ratio(good, ref, mag) <= W.c_separable(K) and W.rel_err(good, ref) <= 1e-6
        assert W.worst_ratio(leaky, ref, mag) > 1000 * W.c_separable(K)          # caught at every scale
        assert (W.rel_err(leaky, ref) <= 1e-6) == hidden


def test_worst_ratio_compares_every_element():
    ref = np.array([1.0, 1e-6, 0.0, -3.0])
    mag = np.array([2.0, 1e-6, 0.0, 3.0])
    assert W.worst_ratio(ref, ref, mag) == 0.0
    got = ref.copy()
    got[1] += 5 * W.UNIT * 1e-6                       # five units of that element's own magnitude: 3e-13 of the tensor max
    assert abs(W.worst_ratio(got, ref, mag) - 5.0) < 1e-6 and W.rel_err(got, ref) < 1e-12
    got = ref.copy()
    got[2] = 1e-30                                    # a voxel no term contributes to must be exactly zero
    assert W.worst_ratio(got, ref, mag) == np.inf
    with pytest.raises(AssertionError):
        W.worst_ratio(np.array([np.nan]), np.array([0.0]), np.array([1.0]))
    with pytest.raises(AssertionError):
        W.worst_ratio(np.zeros(3), np.zeros(4), np.zeros(4))


def test_reference_magnitudes():
    """mag is the oracle on absolute values: it bounds |ref|, and for the adjoint it is the gradient of the all-absolute
    loss, factor gradients and folded penalties included."""
    rng = np.random.default_rng(5)
    d, t, C = (2, 3, 4), (5, 7, 9), 3
    _, frev = W.filters(4)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    lll, hf, g = f(C, *d), f(C, 7, *d), f(C, *t)
    ml, mh = torch.from_numpy(rng.uniform(-1, 1, d).astype(np.float32)), torch.from_numpy(rng.uniform(-1, 1, (7,) + d).astype(np.float32))
    pen = [0.7, -1.3, 0.4, 2.1]
    for thr in (None, 0.5):
        r = W.level_reference(lll, hf, frev, t, ml, thr, mh, thr, g, pen)
        assert set(r) == {'out', 'd_lll', 'd_hf', 'd_ml', 'd_mh'}
        for name, (ref, mag) in r.items():
            assert ref.dtype == np.float64 and mag.dtype == np.float64 and ref.shape == mag.shape, name
            assert (np.abs(ref) <= mag * (1 + 1e-12)).all(), name
        # against the fp32 oracle and its autograd (tests/test_wavelets_gpu.py), in the max-normalised metric
        ins = [x.clone().requires_grad_(True) for x in (lll, hf, ml, mh)]
        ap = lambda x, m: x * m.unsqueeze(0) if thr is None else (x * (m >= thr) - x * m).detach() + x * m
        out32 = W.oracle_level64(ap(ins[0], ins[2]), ap(ins[1], ins[3]), frev, t)
        ((out32 * g).sum() + pen[0] * (ins[0] ** 2).sum() + pen[1] * (ins[1] ** 2).sum() + pen[2] * ins[2].abs().sum()
         + pen[3] * ins[3].abs().sum()).backward()
        assert W.rel_err(out32.detach().numpy(), r['out'][0]) <= 1e-6
        for x, name in zip(ins, ('d_lll', 'd_hf', 'd_ml', 'd_mh')):
            assert W.rel_err(x.grad.numpy(), r[name][0]) <= 5e-6, name
    x = f(2, 5, 6, 7)
    ffwd, _ = W.filters(6)
    ref, mag = W.encode_reference(x, ffwd)
    assert ref.dtype == np.float64 and ref.shape == (2, 8, 5, 5, 6) and (np.abs(ref) <= mag * (1 + 1e-12)).all()


def test_header_states_the_limits():
    import os
    import re
    header = open(os.path.join(os.path.dirname(W.GOLD), '..', 'include', 'lfgc.h')).read()
    for table in (W.SYNTHESIS_MAX_D2, W.DWT_MAX_N2):
        row = r'\s+'.join('L = %d: %d' % (L, table[L]) for L in (2, 4, 6, 8))
        assert re.search(row, header), row
    assert 'd2 = %s)' % ', '.join(str(W.ADJOINT_MAX_D2[L]) for L in (2, 4, 6, 8)) in header
