"""GPU tests for the codec writer's label widths 1 to 16: the label packer bit for bit against the
reference READER's slicing rule (oracle/ref_codec.py), the sorted-value k-means for up to 65 536 centres against the same
Lloyd step in numpy, files written at other widths read back by the oracle and by restore_model, codebook quality against
the reference's own scikit-learn clustering (recorded by tools/make_goldens_codec_bits.py), and restore_model for a basis
other than db2."""
import ctypes
import functools
import json
import os
import time

import numpy as np
import pytest
import torch

from oracle import ref_codec as K
from test_hip_forward import GOLD, dev  # noqa: F401

pytestmark = pytest.mark.gpu

KS = [512, 4096, 8192, 65536]           # all midpoints in LDS (<= 8192) and the two-level search; 65 536 > the 53 002 values


def bit_matrix_bytes(labels, bits):
    """np.packbits of the MSB-first bit matrix: the stream with a LEFT-aligned tail (zero bits on the right)."""
    w = (np.asarray(labels, np.int64)[:, None] >> np.arange(bits - 1, -1, -1)[None, :]) & 1
    return np.packbits(w.reshape(-1).astype(np.uint8))


# ---- 1. packer -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('bits', [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 16])
def test_pack_labels_bit_for_bit(dev, bits):
    from latent_feature_grid_compression_amd import ops
    rng = np.random.default_rng(100 + bits)
    for n in (1, 2, 7, 8, 9, 63, 64, 65, 1003, 2049, 100003):
        labels = rng.integers(0, 1 << bits, n)
        want = bit_matrix_bytes(labels, bits)
        dtypes = [np.uint16] if bits > 8 else [np.uint8, np.uint16]
        for dt in dtypes:
            got = ops.codec_pack_labels(torch.from_numpy(labels.astype(dt)).to(dev), bits).cpu().numpy()
            assert got.dtype == np.uint8 and got.size == (n * bits + 7) // 8
            assert np.array_equal(got, want), (n, bits, dt)
            assert np.array_equal(K.unpack_labels(got.tobytes(), n, bits), labels), (n, bits)    # EVERY label, the reader's rule
            if (n * bits) % 8 == 0:
                assert got.tobytes() == K.pack_labels(labels, bits)                              # no tail: the reference's bytes
            top = 8 * np.dtype(dt).itemsize
            if bits < top:                                                                       # junk above `bits` is masked
                junk = (labels | (rng.integers(1, 1 << (top - bits), n) << bits)).astype(dt)
                got = ops.codec_pack_labels(torch.from_numpy(junk).to(dev), bits).cpu().numpy()
                assert np.array_equal(got, want), (n, bits, dt, 'junk')


# ---- 2. / 3. the Lloyd iteration ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lloyd_data():
    """The data of test_hip_codec.py::test_kmeans_is_lloyd_from_the_ward_init: 53 002 values, shuffled."""
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.standard_normal(50000) * 0.1, rng.standard_normal(3000) * 2.0, [7.5, -9.0]]).astype(np.float32)
    rng.shuffle(x)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ward_init(k):
    from latent_feature_grid_compression_amd import _lib
    s = np.sort(lloyd_data())
    init = np.empty(k, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    assert _lib.load().lfgc_codec_ward_init_host(s.ctypes.data_as(fp), s.size, k, init.ctypes.data_as(fp)) == 0
    init.setflags(write=False)
    return init


def wide_midpoints(c):
    """The midpoints of lfgc_codec_kmeans1d_sorted_f32 (include/lfgc.h): fp32 0.5 (c[j] + c[j+1]), moved one float down where
    rounding put it onto c[j+1] > c[j]."""
    mid = 0.5 * (c[:-1] + c[1:])
    assert mid.dtype == np.float32
    return np.where((mid >= c[1:]) & (c[:-1] < c[1:]), np.nextafter(c[1:], c[:-1]), mid)


def nearest_distance(x, c):
    """|x - nearest entry of the sorted codebook c| in fp64."""
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    i = np.clip(np.searchsorted(c64, x64), 1, c64.size - 1)
    return np.minimum(np.abs(x64 - c64[i - 1]), np.abs(x64 - c64[i]))


def wcss(x, c):
    return float(np.sum(nearest_distance(x, c) ** 2))


@pytest.mark.parametrize('k', KS)
def test_one_lloyd_step_against_numpy(dev, k):
    """One step, not 25: after many steps a one-ulp difference can move a value across a midpoint.  Both sides round an fp64
    mean that differs only in summation order: one fp32 ulp."""
    from latent_feature_grid_compression_amd import ops
    x, init = lloyd_data(), ward_init(k)
    mid = 0.5 * (init[:-1] + init[1:])
    assert mid.dtype == np.float32
    a = np.searchsorted(mid, x, side='left')
    sums = np.bincount(a, weights=x.astype(np.float64), minlength=k)
    cnt = np.bincount(a, minlength=k)
    ref = np.where(cnt > 0, (sums / np.maximum(cnt, 1)).astype(np.float32), init)
    xs = torch.from_numpy(np.sort(x)).to(dev)
    got = ops.codec_kmeans_sorted(xs, torch.from_numpy(init.copy()).to(dev), iterations=1).cpu().numpy()
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    print('k %d: %d empty clusters, max |centre - numpy| / ulp = %.2f' % (k, int((cnt == 0).sum()), float((err / np.spacing(np.abs(ref))).max())))
    assert np.all(err <= np.spacing(np.abs(ref)))
    assert np.array_equal(got[cnt == 0], init[cnt == 0])                       # an empty cluster keeps its centre exactly
    # the labels of the unsorted values follow the same counting rule against the new centres
    lab = ops.codec_labels_u16(torch.from_numpy(x.copy()).to(dev), torch.from_numpy(got).to(dev))
    assert lab.dtype == torch.uint16
    assert np.array_equal(lab.cpu().numpy(), np.searchsorted(wide_midpoints(got), x, side='left'))
    # iterations = 0 leaves the centres alone
    same = ops.codec_kmeans_sorted(xs, torch.from_numpy(init.copy()).to(dev), iterations=0).cpu().numpy()
    assert np.array_equal(same, init)


@pytest.mark.parametrize('k', KS)
def test_lloyd_properties(dev, k):
    from latent_feature_grid_compression_amd import ops
    x, init = lloyd_data(), ward_init(k)
    xt = torch.from_numpy(x.copy()).to(dev)
    xs = torch.sort(xt)[0]
    runs = []
    for _ in range(2):
        c = ops.codec_kmeans_sorted(xs, torch.from_numpy(init.copy()).to(dev), iterations=40)
        runs.append((c.cpu().numpy(), ops.codec_labels_u16(xt, c).cpu().numpy()))
    (c, lab), (c2, lab2) = runs
    assert np.array_equal(c, c2) and np.array_equal(lab, lab2)                 # deterministic
    assert c.size == k and np.all(np.diff(c) >= 0)
    d = np.abs(x.astype(np.float64) - c.astype(np.float64)[lab])
    assert np.all(d - nearest_distance(x, c) <= 1e-7 * np.abs(x).max())
    w0, w1 = wcss(x, init), wcss(x, c)
    print('k %d: within-cluster sum of squares %.6e -> %.6e' % (k, w0, w1))
    assert w1 <= w0 * (1 + 1e-12)                                              # Lloyd is monotone; slack for rounding only
    # the public entry (sort + strided sample + Ward + Lloyd + labels) agrees with itself too
    p1, p2 = ops.codec_kmeans(xt, k), ops.codec_kmeans(xt, k)
    assert p1[1].dtype == torch.uint16 and torch.equal(p1[0], p2[0])
    assert np.array_equal(p1[1].cpu().numpy(), p2[1].cpu().numpy())


# ---- 4. degenerate inputs ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', ['3 values', '5000 values', '100 distinct', 'all equal'])
def test_degenerate_inputs_are_reproduced_exactly(dev, case):
    from latent_feature_grid_compression_amd import ops
    rng = np.random.default_rng(12)
    if case == '3 values':
        x, k = np.asarray([0.5, -1.0, 0.25], np.float32), 65536
    elif case == '5000 values':
        x, k = rng.standard_normal(5000).astype(np.float32), 8192
    elif case == '100 distinct':
        x, k = rng.standard_normal(100).astype(np.float32)[rng.integers(0, 100, 20000)], 4096
    else:
        x, k = np.full(3000, 0.375, np.float32), 512
    centres, labels = ops.codec_kmeans(torch.from_numpy(x).to(dev), k)
    c, lab = centres.cpu().numpy(), labels.cpu().numpy()
    assert labels.dtype == torch.uint16 and c.size == k and np.all(np.diff(c) >= 0)
    assert np.array_equal(c[lab], x)


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------------

def small_model(dev, wavelet='db2'):
    """The shape of test_hip_codec.py::test_restore_reads_other_label_widths: C = 3, G = 15, H = 16, L = 3, 40 % pruned."""
    from latent_feature_grid_compression_amd.model.model_utils import setup_model
    C, G, H, L = 3, 15, 16, 3
    torch.manual_seed(5)
    m = setup_model(3, H, 1, L, 'fourier', 2, '', 0.1, 0.9, wavelet, C, G, '')
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for p in m.feature_grid:
            p.copy_(torch.randn(p.shape, generator=g) * (torch.rand(p.shape, generator=g) > 0.4).float())
    return m.to(dev), L


def check_file_against_model(m, L, raw, mask_raw, bits):
    """The oracle's reading of a file we wrote against the model it was written from.  Returns the parse."""
    got = K.parse(raw, mask_raw)                                                # asserts that no byte is left over
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    grids = [sd['feature_grid.%d' % i].reshape(-1) for i in range(len(m.feature_grid))]
    assert got['header']['bit_precision'] == bits
    assert got['header']['grid_sizes'] == [int(np.count_nonzero(g)) for g in grids]
    assert mask_raw == np.packbits(np.concatenate(grids) != 0).tobytes()
    for i in (0, L):                                                           # fp32 layers: identical bytes
        name = 'net_layers.%d' % i if i < L else 'final_layer'
        assert np.array_equal(got['weights'][i], sd[name + '.weight'].reshape(-1))
        assert np.array_equal(got['biases'][i], sd[name + '.bias'])
    for i in range(1, L):
        assert np.array_equal(got['biases'][i], sd['net_layers.%d.bias' % i])
    originals = [sd['net_layers.%d.weight' % i].reshape(-1) for i in range(1, L)] + [g[g != 0] for g in grids]
    assert len(got['blocks']) == len(originals)
    size = 9 + 8 * len(grids) + 4 * sum(got['weights'][i].size + got['biases'][i].size for i in (0, L)) + \
        4 * sum(got['biases'][i].size for i in range(1, L))
    for b, x in zip(got['blocks'], originals):
        c = b['centres']
        assert c.size == 1 << bits and np.all(np.diff(c) >= 0) and b['labels'].size == x.size
        d = np.abs(x.astype(np.float64) - c.astype(np.float64)[b['labels']])
        assert np.all(d - nearest_distance(x, c) <= 1e-7 * np.abs(x).max())
        size += 4 * c.size + (x.size * bits + 7) // 8 + (4 if bits % 8 else 0)
    assert len(raw) == size
    return got


def check_restored_against_parse(back, got, L):
    sd = back.state_dict()
    for i, g in enumerate(got['grids']):
        assert np.array_equal(sd['feature_grid.%d' % i].cpu().numpy().reshape(-1), g)
    for i in range(L):
        assert np.array_equal(sd['net_layers.%d.weight' % i].cpu().numpy().reshape(-1), got['weights'][i])
        assert np.array_equal(sd['net_layers.%d.bias' % i].cpu().numpy(), got['biases'][i])
    assert np.array_equal(sd['final_layer.weight'].cpu().numpy().reshape(-1), got['weights'][L])
    assert np.array_equal(sd['final_layer.bias'].cpu().numpy(), got['biases'][L])


@pytest.mark.parametrize('bits', [1, 3, 5, 8, 11, 16])
def test_store_at_other_widths_end_to_end(dev, tmp_path, bits):
    from latent_feature_grid_compression_amd.model.model_utils import restore_model, store_model_parameters
    m, L = small_model(dev)
    path = str(tmp_path / ('bits%d' % bits))
    store_model_parameters(m, path, bits)
    raw, mask_raw = open(path, 'rb').read(), open(path + '_mask.bnr', 'rb').read()
    got = check_file_against_model(m, L, raw, mask_raw, bits)
    check_restored_against_parse(restore_model(path), got, L)
    if bits == 8:                                                              # the default is 8 and its files are unchanged
        store_model_parameters(m, path + '_default')
        assert open(path + '_default', 'rb').read() == raw
        assert open(path + '_default_mask.bnr', 'rb').read() == mask_raw


# ---- 6. quality against the reference's own clustering ----------------------------------------------------------------------------

def quality_input(name, gold):
    if name == 'laplace':
        lp = gold['laplace']
        return np.random.default_rng(lp['seed']).laplace(0, lp['scale'], lp['n']).astype(np.float32)
    g = np.load(os.path.join(GOLD, 'codec_small.npz'))['sd.feature_grid.2'].reshape(-1)
    return g[g != 0].astype(np.float32)


def our_mse(dev, x, bits):
    from latent_feature_grid_compression_amd import ops
    centres, labels = ops.codec_kmeans(torch.from_numpy(x).to(dev), 1 << bits)
    rec = centres.cpu().numpy()[labels.cpu().numpy()]
    return float(np.mean((rec.astype(np.float64) - x.astype(np.float64)) ** 2))


@pytest.mark.parametrize('name', ['codec_small.feature_grid.2', 'laplace'])
def test_codebook_quality_against_the_reference_clustering(dev, name):
    """Margin and reason as in test_store_writes_the_reference_format: the reference's clustering (scikit-learn
    KMeans(n_init=4)) is unseeded, so its recorded error is one draw."""
    gold = json.load(open(os.path.join(GOLD, 'codec_bits_mse.json')))
    x = quality_input(name, gold)
    assert x.size == gold['n'][name]
    for bits in gold['bits']:
        mse_ref = gold['mse'][name][str(bits)]
        mse_ours = our_mse(dev, x, bits)
        print('%s, %d bits: mse %.4e, reference %.4e' % (name, bits, mse_ours, mse_ref))
        assert mse_ours <= 1.25 * mse_ref + 1e-12, (bits, mse_ours, mse_ref)


@pytest.mark.parametrize('bits', [14, 16])
def test_codebook_quality_sanity_cap_beyond_the_reference(dev, bits):
    """No reference value here (scikit-learn does not finish k = 16 384 on 50 000 points in useful time).  A SANITY CAP only:
    the error of a uniform quantiser with 2^bits steps over the value range, which any sensible codebook beats."""
    gold = json.load(open(os.path.join(GOLD, 'codec_bits_mse.json')))
    x = quality_input('laplace', gold)
    mse = our_mse(dev, x, bits)
    cap = ((float(x.max()) - float(x.min())) / 2 ** bits) ** 2 / 12
    print('laplace, %d bits: mse %.4e, uniform quantiser %.4e' % (bits, mse, cap))
    assert mse <= cap


# ---- 7. other bases ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('bits', [8, 11])
def test_haar_model_round_trip(dev, tmp_path, bits):
    from latent_feature_grid_compression_amd.model.model_utils import restore_model, store_model_parameters
    m, L = small_model(dev, 'haar')
    path = str(tmp_path / ('haar%d' % bits))
    store_model_parameters(m, path, bits)
    got = check_file_against_model(m, L, open(path, 'rb').read(), open(path + '_mask.bnr', 'rb').read(), bits)
    back = restore_model(path, wavelet_filter='haar')
    assert np.array_equal(back.shape_array, m.shape_array)
    check_restored_against_parse(back, got, L)
    back.train()
    with torch.no_grad():
        assert torch.isfinite(back(torch.rand(500, 3, device=dev) * 2 - 1)).all()
    with pytest.raises(ValueError, match='wavelet_filter'):                    # db2 coefficient shapes differ: named, not .view
        restore_model(path)


# ---- 8. cfg-3 size --------------------------------------------------------------------------------------------------------------------------

def test_cfg3_sized_round_trip_at_other_widths(dev, tmp_path):
    """cfg-3 coefficient count (9.6 M, a third pruned) as test_hip_codec.py::test_cfg3_sized_round_trip_and_timing builds it, at
    8 bits (the baseline of the error comparison) and 4, 12, 16."""
    from latent_feature_grid_compression_amd.model.model_utils import setup_model, store_model_parameters, restore_model
    torch.manual_seed(3)
    m = setup_model(3, 128, 1, 4, 'fourier', 2, '', 0.1, 0.9, 'db2', 32, 64, '').to(dev)
    with torch.no_grad():
        for p in m.feature_grid:
            p.mul_((torch.rand_like(p) > 0.33).float())
    rel = {}
    for bits in (8, 4, 12, 16):
        path = str(tmp_path / ('cfg3_%d' % bits))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        store_model_parameters(m, path, bits)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        back = restore_model(path)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        num = den = 0.0
        for a, b in zip(m.feature_grid, back.feature_grid):
            a, b = a.detach(), b.detach()
            assert torch.equal(a == 0, b == 0)                                 # the pruning pattern survives exactly
            assert torch.unique(b).numel() <= (1 << bits) + 1
            num += (a - b).double().square().sum().item()
            den += a.double().square().sum().item()
        rel[bits] = (num / den) ** 0.5
        print('cfg3 codec, %2d bits: store %.3f s, restore %.3f s, file %.1f MB, rms error / rms %.2e' % (
            bits, t1 - t0, t2 - t1, os.path.getsize(path) / 1e6, rel[bits]))
        os.remove(path)
    assert rel[12] <= rel[8] and rel[16] <= rel[8]
