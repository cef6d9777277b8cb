"""GPU tests of the SSIM kernel (lfgc_ssim_planes_f32) and its drivers against the NumPy fp64 reference (tests/ssim_ref.py).

Tolerance for every map value, every plane sum and every mean: 1e-9 absolute.  For |data| <= 1 and L >= 1 a moment summed
over at most 16^3 terms carries at most about 5e-13 of rounding and each factor of the formula is at least C1 >= 1e-4, so
any fp64 summation order stays below 5e-9 relative in the worst (flat) window and orders of magnitude lower in practice;
fp32 accumulation misses the bound (5e-8 .. 2e-6).  The test data therefore has |values| <= 1 and a range of at least 1.
Equal contents give exactly 1.0, and plane sums are compared bit for bit across sub-volume calls."""
import ctypes

import numpy as np
import pytest
import torch

import ssim_ref as SR
from test_hip_forward import build_synth, dev  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-9
_ROWS = 3                  # sentinel planes after every output
_SENTINEL = -77.0
L_RANGE = 2.0              # the data lies in [-1, 1]
C1, C2 = SR.constants(L_RANGE)


def _sim():
    from latent_feature_grid_compression_amd.visualization import Similarity
    return Similarity


def _ops():
    from latent_feature_grid_compression_amd import ops
    return ops


def _weights(spec):
    """7 -> three uniform axes of 7; 'g11' -> three Gaussian axes of 11; a tuple -> one uniform axis per entry."""
    S = _sim()
    if spec == 'g11':
        return [S.ssim_weights(11, True, 1.5)] * 3
    if isinstance(spec, tuple):
        return [S.ssim_weights(w) for w in spec]
    return [S.ssim_weights(spec)] * 3


def _entry_with_sentinels(a, b, weights, strides, c1, c2, k, dev_, want_map=True):
    """The C entry through the binding itself; outputs and workspace carry sentinel rows that must stay untouched."""
    from latent_feature_grid_compression_amd import _lib
    lib = _lib.load()
    ta, tb = torch.from_numpy(a).to(dev_), torch.from_numpy(b).to(dev_)
    n = a.shape
    lengths = [len(g) for g in weights]
    m = [(nn - w) // s + 1 for nn, w, s in zip(n, lengths, strides)]
    w_arr, s_arr = (ctypes.c_int * 3)(*lengths), (ctypes.c_int * 3)(*strides)
    flat = np.concatenate(weights)
    g = (ctypes.c_double * flat.size)(*flat.tolist())
    nbytes = lib.lfgc_ssim_workspace_bytes(n[0], n[1], n[2], w_arr, s_arr)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.full((nbytes // 8 + _ROWS,), _SENTINEL, dtype=torch.float64, device=dev_)
    sums = torch.full((m[0] + _ROWS,), _SENTINEL, dtype=torch.float64, device=dev_)
    smap = torch.full((m[0] + _ROWS, m[1], m[2]), _SENTINEL, dtype=torch.float64, device=dev_)
    _lib.check(lib.lfgc_ssim_planes_f32(ta.data_ptr(), tb.data_ptr(), n[0], n[1], n[2], g, w_arr, s_arr, c1, c2, k, sums.data_ptr(),
                                        smap.data_ptr() if want_map else None, ws.data_ptr(), nbytes,
                                        torch.cuda.current_stream(dev_).cuda_stream), 'ssim')
    torch.cuda.synchronize()
    for t, rows in ((ws, nbytes // 8), (sums, m[0]), (smap, m[0] if want_map else 0)):
        assert bool((t[rows:] == _SENTINEL).all())                             # nothing written past the outputs
    return smap[:m[0]].cpu().numpy(), sums[:m[0]].cpu().numpy()


# array shape, windows, strides, cov_norm -- the smallest shapes that can break a tile (8 x 32 windows), a halo or a tail
CASES = [
    ((1, 1, 1), 1, (1, 1, 1), 1.0),               # the smallest possible
    ((7, 7, 7), 7, (1, 1, 1), 1.0),               # one window
    ((7, 7, 70), 7, (1, 1, 1), 1.0),              # 64 windows along z
    ((7, 8, 71), 7, (1, 1, 1), 1.0),              # 65 windows along z
    ((7, 9, 69), 7, (1, 1, 1), 1.0),              # 63 windows along z
    ((9, 10, 23), 7, (1, 1, 1), 1.0),             # odd extents
    ((12, 13, 29), 'g11', (1, 1, 1), 1.0),        # Gaussian weights
    ((11, 11, 11), 'g11', (1, 1, 1), 1.0),        # one Gaussian window
    ((16, 16, 17), 16, (1, 1, 1), 1.0),           # the longest window
    ((16, 9, 20), 7, (2, 2, 2), 1.0),             # stride 2
    ((8, 17, 70), 8, (3, 3, 3), 1.0),             # stride does not divide
    ((6, 11, 13), 2, (5, 5, 5), 1.0),             # stride longer than the window
    ((3, 12, 140), (1, 11, 11), (1, 1, 1), 1.0),  # the image layout
    ((5, 40, 6), (3, 7, 2), (1, 2, 1), 1.0),      # anisotropic windows
    ((9, 10, 23), 7, (1, 1, 1), 343.0 / 342.0),   # the sample covariance
    ((8, 42, 40), 7, (7, 7, 7), 1.0),             # the staged plane of 8 x 32 windows passes 60 KB: tiles of 4 x 32, two of them
    ((16, 52, 340), 16, (20, 20, 20), 1.0),       # the smallest tiles, 1 x 16, with gaps between the windows: 2 x 2 of them
]


@pytest.mark.parametrize('sigma', [0.05, 0.5])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_map_and_plane_sums_equal_the_reference(dev, case, sigma):
    shape, spec, strides, k = CASES[case]
    a, b = SR.make_field(shape, sigma, 10 + case)
    assert np.abs(a).max() <= 1.0 and np.abs(b).max() <= 1.0
    weights = _weights(spec)
    want_map, want_sums = SR.ssim_map(a, b, weights, strides, C1, C2, k)
    got_map, got_sums = _entry_with_sentinels(a, b, weights, strides, C1, C2, k, dev)
    assert got_map.shape == want_map.shape
    print('case %d sigma %g: max |map - ref| %.3e, max |plane sum - ref| %.3e, values %.3f .. %.3f'
          % (case, sigma, np.abs(got_map - want_map).max(), np.abs(got_sums - want_sums).max(), want_map.min(), want_map.max()))
    assert np.abs(got_map - want_map).max() <= TOL
    assert np.abs(got_sums - want_sums).max() <= TOL
    _, only_sums = _entry_with_sentinels(a, b, weights, strides, C1, C2, k, dev, want_map=False)
    assert np.array_equal(only_sums, got_sums)                                 # the map is optional and changes nothing


def test_values_spread_over_the_range():
    """The data of the cases above does not sit near 1 only (host arithmetic; here because it qualifies the GPU cases)."""
    lo, hi = [], []
    for sigma in (0.05, 0.5):
        a, b = SR.make_field((9, 10, 23), sigma, 15)
        smap, _ = SR.ssim_map(a, b, _weights(7), (1, 1, 1), C1, C2)
        lo.append(smap.min())
        hi.append(smap.max())
    assert min(lo) < 0.3 and max(hi) > 0.9


@pytest.mark.parametrize('case', [0, 3, 8, 10, 11, 12, 13, 14, 15, 16])
def test_equal_contents_give_exactly_one(dev, case):
    shape, spec, strides, k = CASES[case]
    a, _ = SR.make_field(shape, 0.5, 40 + case)
    got_map, got_sums = _entry_with_sentinels(a, a.copy(), _weights(spec), strides, C1, C2, k, dev)   # two buffers
    assert np.all(got_map == 1.0)
    assert np.all(got_sums == got_map.shape[1] * got_map.shape[2])


@pytest.mark.parametrize('strides', [(1, 1, 1), (2, 2, 2)])
def test_nan_stays_in_the_windows_that_cover_it(dev, strides):
    shape, at = (9, 10, 23), (4, 3, 11)
    a, b = SR.make_field(shape, 0.5, 50)
    weights = _weights(7)
    want_map, want_sums = SR.ssim_map(a, b, weights, strides, C1, C2)
    a[at] = np.nan
    cover = SR.covering_windows(at, shape, (7, 7, 7), strides)
    assert cover.any() and not cover.all()
    got_map, got_sums = _entry_with_sentinels(a, b, weights, strides, C1, C2, 1.0, dev)
    assert np.array_equal(np.isnan(got_map), cover)
    assert np.abs(got_map[~cover] - want_map[~cover]).max() <= TOL
    plane_nan = cover.any(axis=(1, 2))
    assert np.array_equal(np.isnan(got_sums), plane_nan)
    if (~plane_nan).any():
        assert np.abs(got_sums[~plane_nan] - want_sums[~plane_nan]).max() <= TOL


# ---- slab independence, bit for bit ---------------------------------------------------------------------------------------

_SLAB_SHAPE = (23, 10, 19)


@pytest.mark.parametrize('stride', [1, 2])
def test_plane_sums_do_not_depend_on_the_sub_volume(dev, stride):
    ops = _ops()
    a, b = SR.make_field(_SLAB_SHAPE, 0.5, 60)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    weights, strides, w = _weights(7), (stride,) * 3, 7
    whole, whole_map = ops.ssim_plane_sums(ta, tb, weights, strides, C1, C2, want_map=True)
    m0 = whole.numel()
    assert m0 == (_SLAB_SHAPE[0] - w) // stride + 1
    _, want_sums = SR.ssim_map(a, b, weights, strides, C1, C2)
    assert np.abs(whole.cpu().numpy() - want_sums).max() <= TOL
    cuts = [(p, p + 1) for p in range(m0)] + [(p, p + 2) for p in range(m0 - 1)] + [(0, 3), (0, m0 - 1), (m0 - 3, m0), (1, m0)]
    for p0, p1 in cuts:
        x0, x1 = p0 * stride, (p1 - 1) * stride + w
        part, part_map = ops.ssim_plane_sums(ta[x0:x1], tb[x0:x1], weights, strides, C1, C2, want_map=True)
        assert part.numel() == p1 - p0
        assert torch.equal(part, whole[p0:p1]), (p0, p1)
        assert torch.equal(part_map, whole_map[p0:p1]), (p0, p1)


@pytest.mark.parametrize('stride', [1, 2])
def test_volume_ssim_does_not_depend_on_the_slab_size(dev, stride):
    S = _sim()
    a, b = SR.make_field(_SLAB_SHAPE, 0.5, 61)
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    plane, w = _SLAB_SHAPE[1] * _SLAB_SHAPE[2], 7
    L = float(b.max()) - float(b.min())
    want_map, _ = SR.ssim_map(a, b, _weights(7), (stride,) * 3, *SR.constants(L))
    means = []
    for planes_per_slab in (1, 3, None):
        limit = 1 << 24 if planes_per_slab is None else plane * ((planes_per_slab - 1) * stride + w)
        assert len(S.ssim_slabs(_SLAB_SHAPE[0], plane, w, stride, limit)) == \
            (1 if planes_per_slab is None else -(-want_map.shape[0] // planes_per_slab))
        mean, smap = S.volume_ssim(ta, tb, window=7, stride=stride, max_slab_voxels=limit, return_map=True)
        assert np.abs(smap.cpu().numpy() - want_map).max() <= TOL
        means.append(mean)
        assert S.volume_ssim(ta, tb, window=7, stride=stride, max_slab_voxels=limit) == mean
    assert means[0] == means[1] == means[2]
    assert abs(means[0] - want_map.mean()) <= TOL
    assert S.volume_ssim(ta, ta.clone(), window=7, stride=stride, data_range=L, max_slab_voxels=plane * 9) == 1.0
    # scikit-image's default numbers: the sample covariance of a uniform window
    k_mean = S.volume_ssim(ta, tb, window=7, stride=stride, sample_covariance=True)
    k_map, _ = SR.ssim_map(a, b, _weights(7), (stride,) * 3, *SR.constants(L), 343.0 / 342.0)
    assert abs(k_mean - k_map.mean()) <= TOL and k_mean != means[0]


# ---- the model against the ground truth -------------------------------------------------------------------------------------

def test_ssim_from_net(dev):
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    from latent_feature_grid_compression_amd.visualization.OutputToVTK import field_from_net_fused
    S = _sim()
    res = (20, 12, 18)
    net, _ = build_synth(4, 15, 16, 3, 7, dev)
    net = net.eval()
    ds = IndexDataset(res, 16, build_index_table=False)
    _, gt = SR.make_field(res, 0.5, 62)
    gt_dev = torch.from_numpy(gt).to(dev)
    pred = field_from_net_fused(ds, net).cpu().numpy()
    assert pred.shape == res and np.abs(pred).max() <= 1.0
    L = float(gt.max()) - float(gt.min())
    assert L >= 1.0
    want_map, _ = SR.ssim_map(pred, gt, _weights(7), (1, 1, 1), *SR.constants(L))
    plane = res[1] * res[2]
    one = S.ssim_from_net(ds, net, gt_dev, max_slab_voxels=plane * 7)          # one origin plane per slab
    mean, smap = S.ssim_from_net(ds, net, gt_dev, return_map=True)              # the whole volume at once
    print('ssim_from_net: %.12f, reference %.12f' % (mean, want_map.mean()))
    assert np.abs(smap.cpu().numpy() - want_map).max() <= TOL
    assert abs(mean - want_map.mean()) <= TOL
    assert one == mean
    assert S.ssim_from_net(ds, net, gt_dev, max_slab_voxels=plane * 10) == mean
    with pytest.raises(ValueError, match='eval'):
        S.ssim_from_net(ds, net.train(), gt_dev)
    net.eval()
    with pytest.raises(ValueError, match='shape'):
        S.ssim_from_net(ds, net, gt_dev[:19])


# ---- renders ------------------------------------------------------------------------------------------------------------------

def test_image_ssim(dev):
    from latent_feature_grid_compression_amd.visualization import Render
    S = _sim()
    height, width, C = 12, 14, 4
    rng = np.random.default_rng(63)
    x = rng.random((height * width, C), dtype=np.float32)
    y = np.clip(x + 0.2 * rng.standard_normal((height * width, C)).astype(np.float32), 0.0, 1.0)
    planes = [np.ascontiguousarray(t.reshape(height, width, C).transpose(2, 0, 1)) for t in (x, y)]
    g = S.ssim_weights(11, True, 1.5)
    want_map, _ = SR.ssim_map(planes[0], planes[1], [np.ones(1), g, g], (1, 1, 1), *SR.constants(1.0))
    assert want_map.shape == (C, 2, 4)
    tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    got = Render.image_ssim(tx, ty, width, height)
    print('image_ssim: %.12f, reference %.12f' % (got, want_map.mean()))
    assert abs(got - want_map.mean()) <= TOL
    assert S.image_ssim(tx, tx.clone(), width, height) == 1.0
    uni = S.image_ssim(tx, ty, width, height, window=7, gaussian=False)
    u = S.ssim_weights(7)
    want_uni, _ = SR.ssim_map(planes[0], planes[1], [np.ones(1), u, u], (1, 1, 1), *SR.constants(1.0))
    assert abs(uni - want_uni.mean()) <= TOL
