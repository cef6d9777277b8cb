"""Host tests of the SSIM feature (no GPU): the NumPy reference (tests/ssim_ref.py) against closed forms, its separable
evaluation and scipy; ssim_weights; the slab cuts of Similarity.volume_ssim with the device call replaced by the reference;
the ValueError cases on CPU tensors; and the argument errors of the C entry, which are decided before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import ssim_ref as SR
from latent_feature_grid_compression_amd import _lib, ops
from latent_feature_grid_compression_amd._lib import LfgcError
from latent_feature_grid_compression_amd.visualization import Render, Similarity

E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4, -5
C1, C2 = SR.constants(2.0)


def _uniform(w):
    return [Similarity.ssim_weights(w)] * 3


# ---- the reference ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('p,q', [(0.5, -0.25), (1.0, 1.0), (0.0, 0.75)])
def test_reference_on_constant_arrays(p, q):
    a = np.full((6, 7, 8), p, np.float32)
    b = np.full((6, 7, 8), q, np.float32)
    smap, sums = SR.ssim_map(a, b, _uniform(4), (1, 2, 1), C1, C2)
    assert smap.shape == (3, 2, 5)
    # both variances and the covariance vanish up to rounding of the moments (<= 1e-15 against C2 = 3.6e-3)
    np.testing.assert_allclose(smap, (2 * p * q + C1) / (p * p + q * q + C1), rtol=0, atol=1e-12)
    np.testing.assert_allclose(sums, smap.sum(axis=(1, 2)), rtol=0, atol=1e-12)


def test_reference_equal_inputs_give_exactly_one():
    a, _ = SR.make_field((9, 10, 11), 0.5, 1)
    for weights in (_uniform(7), [Similarity.ssim_weights(5, True)] * 3):
        smap, sums = SR.ssim_map(a, a.copy(), weights, (1, 1, 2), C1, C2, 343.0 / 342.0)
        assert np.all(smap == 1.0)
        assert np.all(sums == smap.shape[1] * smap.shape[2])


@pytest.mark.parametrize('shape,w,s,gaussian', [((9, 10, 23), 7, 1, False), ((12, 13, 29), 11, 1, True), ((8, 17, 30), 8, 3, False),
                                                ((6, 11, 13), 2, 5, False)])
def test_reference_direct_against_separable(shape, w, s, gaussian):
    a, b = SR.make_field(shape, 0.5, 2)
    weights = [Similarity.ssim_weights(w, gaussian)] * 3
    direct, dsum = SR.ssim_map(a, b, weights, (s,) * 3, C1, C2)
    sep, ssum = SR.ssim_map_separable(a, b, weights, (s,) * 3, C1, C2)
    assert direct.shape == sep.shape
    assert np.abs(direct - sep).max() <= 1e-12
    assert np.abs(dsum - ssum).max() <= 1e-12 * direct.shape[1] * direct.shape[2]
    assert direct.max() - direct.min() > 0.5                   # the data spreads the values, they are not all near 1


def test_reference_against_scipy_uniform_filter():
    ndi = pytest.importorskip('scipy.ndimage')
    a, b = SR.make_field((11, 12, 16), 0.5, 3)
    w = 7
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    lo, hi = w // 2, -(w // 2)
    mom = [ndi.uniform_filter(f, size=w, mode='constant')[lo:hi, lo:hi, lo:hi] for f in (a64, b64, a64 * a64, b64 * b64, a64 * b64)]
    want = SR._ssim(*mom, C1, C2, 1.0)
    got, _ = SR.ssim_map(a, b, _uniform(w), (1, 1, 1), C1, C2)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12


def test_covering_windows():
    cover = SR.covering_windows((4, 0, 6), (9, 10, 23), (7, 7, 7), (1, 1, 2))
    assert cover.shape == (3, 4, 9)
    assert cover[:, 0, :4].all() and cover.sum() == 3 * 1 * 4


# ---- weights ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('size', [1, 2, 7, 11, 16])
@pytest.mark.parametrize('gaussian', [False, True])
def test_ssim_weights(size, gaussian):
    g = Similarity.ssim_weights(size, gaussian, 1.5)
    assert g.dtype == np.float64 and g.shape == (size,)
    assert abs(g.sum() - 1.0) <= 4e-16
    assert np.array_equal(g, g[::-1])
    if gaussian and size > 2:
        assert g[size // 2] == g.max() and g[0] == g.min() and g[0] < g.max()
        x = np.arange(size) - 0.5 * (size - 1)
        np.testing.assert_allclose(g[0] / g[(size - 1) // 2], np.exp(-(x[0] ** 2 - x[(size - 1) // 2] ** 2) / 4.5), rtol=1e-14)
    with pytest.raises(ValueError):
        Similarity.ssim_weights(0)


# ---- slab cuts ----------------------------------------------------------------------------------------------------------

_SHAPE = (23, 10, 19)


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_slab_cuts_cover_every_origin_plane_once(stride):
    n0, plane, w = _SHAPE[0], _SHAPE[1] * _SHAPE[2], 7
    m0 = (n0 - w) // stride + 1
    for limit in [0, 1, plane * w] + [plane * k for k in range(w, n0 + 2)] + [1 << 24]:
        cuts = Similarity.ssim_slabs(n0, plane, w, stride, limit)
        assert [c[0] for c in cuts] == [0] + [c[1] for c in cuts[:-1]] and cuts[-1][1] == m0     # a partition of [0, m0)
        for (p0, p1, x0, x1), nxt in zip(cuts, cuts[1:] + [None]):
            assert p1 > p0 and x0 == p0 * stride and x1 == (p1 - 1) * stride + w and x1 <= n0
            assert (x1 - x0) * plane <= limit or p1 - p0 == 1
            if nxt is not None:
                assert x1 - nxt[2] == w - stride                                                   # the overlap
    assert len(Similarity.ssim_slabs(n0, plane, w, stride, plane * w)) == m0                      # one origin plane each
    assert len(Similarity.ssim_slabs(n0, plane, w, stride, 1 << 24)) == 1


@pytest.mark.parametrize('stride', [1, 2, 3])
def test_volume_ssim_slabs_with_the_reference_as_device(monkeypatch, stride):
    """The device call replaced by the reference: every origin plane is evaluated exactly once, each slab call sees the
    planes its origins need, and the mean equals the reference's whatever the slab size."""
    a, b = SR.make_field(_SHAPE, 0.5, 4)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    calls = []

    def fake(xa, xb, windows, strides, c1, c2, cov_norm=1.0, want_map=False):
        smap, sums = SR.ssim_map(xa.numpy(), xb.numpy(), windows, strides, c1, c2, cov_norm)
        calls.append((xa, smap.shape[0]))
        return torch.from_numpy(sums), (torch.from_numpy(smap) if want_map else None)

    monkeypatch.setattr(ops, 'ssim_plane_sums', fake)
    L = float(b.max()) - float(b.min())
    whole, wsum = SR.ssim_map(a, b, _uniform(7), (stride,) * 3, *SR.constants(L))
    plane = _SHAPE[1] * _SHAPE[2]
    for limit in [plane * 7, plane * 8, plane * 11, plane * 23, 1 << 24]:
        calls.clear()
        mean, smap = Similarity.volume_ssim(ta, tb, window=7, stride=stride, max_slab_voxels=limit, return_map=True)
        assert sum(c[1] for c in calls) == whole.shape[0]
        assert all(c[0].numel() <= limit for c in calls)
        assert np.array_equal(smap.numpy(), whole)             # the reference's taps do not depend on the slab either
        total = 0.0
        for v in wsum.tolist():
            total += v
        assert mean == total / whole.size
    assert len(calls) == 1
    assert Similarity.volume_ssim(ta, tb, window=7, stride=stride, max_slab_voxels=plane * 7) == mean


# ---- argument checks on CPU tensors -------------------------------------------------------------------------------------

def test_value_errors_come_before_the_device_check():
    a = torch.zeros(8, 9, 10)
    b = torch.linspace(-1, 1, 720).reshape(8, 9, 10)
    with pytest.raises(ValueError, match='shape'):
        Similarity.volume_ssim(a, b[:7])
    with pytest.raises(ValueError, match='axis 0'):
        Similarity.volume_ssim(a, b, window=9)
    with pytest.raises(ValueError, match='axis 2'):
        Similarity.volume_ssim(a, b, window=(3, 3, 11))
    with pytest.raises(ValueError, match='stride of axis 1'):
        Similarity.volume_ssim(a, b, window=3, stride=(1, 0, 1))
    with pytest.raises(ValueError, match='1..16'):
        Similarity.volume_ssim(torch.zeros(20, 20, 20), torch.zeros(20, 20, 20), window=17)
    with pytest.raises(ValueError, match='range'):
        Similarity.volume_ssim(b, a)                           # the ground truth is constant: zero range
    with pytest.raises(ValueError, match='shape'):
        ops.ssim_plane_sums(a, b[:7], _uniform(3), (1, 1, 1), C1, C2)
    with pytest.raises(ValueError, match='axis 1'):
        ops.ssim_plane_sums(a, b, [np.ones(3) / 3, np.ones(10) / 10, np.ones(3) / 3], (1, 1, 1), C1, C2)
    with pytest.raises(ValueError, match='stride'):
        ops.ssim_plane_sums(a, b, _uniform(3), (1, 1, -1), C1, C2)
    img = torch.rand(12 * 14, 4)
    with pytest.raises(ValueError, match='shape'):
        Similarity.image_ssim(img, img[:, :3], 14, 12)
    with pytest.raises(ValueError, match='axis 1'):
        Similarity.image_ssim(img, img, 14, 12, window=13)    # longer than the height
    with pytest.raises(ValueError):
        Similarity.image_ssim(img, img, 14, 13)
    assert Render.image_ssim is Similarity.image_ssim


def test_valid_call_on_cpu_tensors_is_refused_like_every_op():
    a = torch.zeros(8, 9, 10)
    b = torch.linspace(-1, 1, 720).reshape(8, 9, 10)
    with pytest.raises(LfgcError, match='no CPU fallback'):
        Similarity.volume_ssim(a, b)
    with pytest.raises(LfgcError, match='no CPU fallback'):
        ops.ssim_plane_sums(a, b, _uniform(7), (1, 1, 1), C1, C2)
    img = torch.rand(12 * 14, 4)
    with pytest.raises(LfgcError, match='no CPU fallback'):
        Similarity.image_ssim(img, img.clone(), 14, 12)


# ---- the C entry: argument errors only, nothing is launched -------------------------------------------------------------

def _call(n=(9, 10, 23), w=(7, 7, 7), s=(1, 1, 1), a=64, b=128, weights=True, sums=256, smap=None, ws=512, ws_bytes=None,
          c=(C1, C2, 1.0), w_null=False, s_null=False):
    """Made-up non-NULL addresses stand for device memory: every case here is refused before anything touches them."""
    lib = _lib.load()
    w_arr, s_arr = (ctypes.c_int * 3)(*w), (ctypes.c_int * 3)(*s)
    need = lib.lfgc_ssim_workspace_bytes(n[0], n[1], n[2], w_arr, s_arr)
    g = (ctypes.c_double * 48)(*([1.0 / 7] * 48))
    return lib.lfgc_ssim_planes_f32(a, b, n[0], n[1], n[2], g if weights else None, None if w_null else w_arr,
                                    None if s_null else s_arr, c[0], c[1], c[2], sums, smap, ws,
                                    need if ws_bytes is None else ws_bytes, None)


def test_c_entry_refuses_before_launching():
    for kw in (dict(a=None), dict(b=None), dict(weights=False), dict(sums=None), dict(ws=None), dict(w_null=True), dict(s_null=True)):
        assert _call(**kw) == E_NULL, kw
    assert _call(n=(6, 10, 23)) == E_SHAPE
    assert _call(n=(9, 10, 6)) == E_SHAPE
    assert _call(w=(7, 0, 7)) == E_SHAPE
    assert _call(s=(1, 1, 0)) == E_SHAPE
    assert _call(c=(0.0, C2, 1.0)) == E_SHAPE
    assert _call(c=(C1, float('nan'), 1.0)) == E_SHAPE
    assert _call(n=(20, 20, 20), w=(7, 17, 7)) == E_UNSUPPORTED
    assert _call(n=(2 ** 31 - 1,) * 3, w=(1, 1, 1)) == E_UNSUPPORTED
    assert _call(ws_bytes=0) == E_WORKSPACE
    need = _lib.load().lfgc_ssim_workspace_bytes(9, 10, 23, (ctypes.c_int * 3)(7, 7, 7), (ctypes.c_int * 3)(1, 1, 1))
    assert need == 3 * 8                                       # 3 origin planes, one 8 x 32 tile each
    assert _call(ws_bytes=need - 1) == E_WORKSPACE
    assert _call(sums=260) == E_ALIGN
    assert _call(smap=1028) == E_ALIGN
    assert _call(ws=516) == E_ALIGN


def test_workspace_bytes():
    lib = _lib.load()

    def need(n, w, s):
        return lib.lfgc_ssim_workspace_bytes(n[0], n[1], n[2], (ctypes.c_int * 3)(*w), (ctypes.c_int * 3)(*s))

    assert need((1, 1, 1), (1, 1, 1), (1, 1, 1)) == 8
    assert need((7, 8, 71), (7, 7, 7), (1, 1, 1)) == 8 * 3     # 2 x 65 windows: one tile row, three tile columns
    assert need((7, 16, 70), (7, 7, 7), (1, 1, 1)) == 8 * 4    # 10 x 64 windows: two tile rows of two tiles
    assert need((23, 10, 19), (7, 7, 7), (2, 2, 2)) == 8 * 9
    assert need((8, 42, 40), (7, 7, 7), (7, 7, 7)) == 8 * 2    # 6 x 5 windows in tiles of 4 x 32: the staged plane is capped
    assert need((16, 52, 340), (16, 16, 16), (20, 20, 20)) == 8 * 4     # 2 x 17 windows in tiles of 1 x 16
    for refused in (((6, 10, 23), (7, 7, 7), (1, 1, 1)), ((9, 10, 23), (7, 0, 7), (1, 1, 1)), ((9, 10, 23), (7, 7, 7), (1, 0, 1)),
                    ((20, 20, 20), (17, 7, 7), (1, 1, 1)), ((2 ** 31 - 1,) * 3, (1, 1, 1), (1, 1, 1))):
        assert need(*refused) == 0, refused
    assert lib.lfgc_ssim_workspace_bytes(9, 10, 23, None, None) == 0
