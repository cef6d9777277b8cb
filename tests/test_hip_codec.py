"""GPU parity tests for the binary checkpoint codec, through the C-ABI.

Pins: files written by the reference's own store_model_parameters and the state its restore_model rebuilt from them
(tests/golden/codec_small.npz), and oracle/ref_codec.py (numpy restatement of the format, itself pinned by the same
files).  Integer / byte work is compared bit for bit.  The codebook VALUES our writer chooses are not comparable with the
reference's (scikit-learn k-means, unseeded there): "parity unpinned" for that one choice -- the test bounds the
quantisation error by the reference's own error on the same tensors instead."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_codec as K
from test_hip_forward import GOLD, dev  # noqa: F401

pytestmark = pytest.mark.gpu


def golden_files(tmp_path):
    g = np.load(os.path.join(GOLD, 'codec_small.npz'))
    path = str(tmp_path / 'binary_model_file')
    with open(path, 'wb') as f:
        f.write(g['param_file'].tobytes())
    with open(path + '_mask.bnr', 'wb') as f:
        f.write(g['mask_file'].tobytes())
    return g, path


def test_restore_reads_reference_written_files(dev, tmp_path):
    from latent_feature_grid_compression_amd.model.model_utils import restore_model
    g, path = golden_files(tmp_path)
    m = restore_model(path)
    sd = m.state_dict()
    keys = [k[9:] for k in g.files if k.startswith('restored.')]
    assert sorted(keys) == sorted(sd.keys())
    for k in keys:
        assert sd[k].is_cuda
        assert np.array_equal(sd[k].cpu().numpy(), g['restored.' + k]), k
    assert np.array_equal(m.shape_array, g['shape_array'])
    # and the rebuilt model runs: same prediction as a model loaded from the reference's restored state
    pos = torch.rand(500, 3, device=dev) * 2 - 1
    m.train()
    with torch.no_grad():
        assert torch.isfinite(m(pos)).all()


def test_store_writes_the_reference_format(dev, tmp_path):
    from latent_feature_grid_compression_amd.model.model_utils import setup_model, store_model_parameters, restore_model
    g, ref_path = golden_files(tmp_path)
    C, G, H, L, nf = [int(v) for v in g['meta']]
    m = setup_model(3, H, 1, L, 'fourier', nf, '', 0.1, 0.9, 'db2', C, G, '')
    m.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('sd.')})
    path = str(tmp_path / 'ours')
    store_model_parameters(m.to(dev), path)
    raw, mask_raw = open(path, 'rb').read(), open(path + '_mask.bnr', 'rb').read()
    assert mask_raw == g['mask_file'].tobytes()                                  # bit mask: byte-identical
    assert len(raw) == g['param_file'].size
    ours = K.parse(raw, mask_raw)                                                # read back by the reference's reader rules
    ref = K.parse(g['param_file'].tobytes(), g['mask_file'].tobytes())
    assert ours['header'] == ref['header']
    for i in (0, L):                                                            # unquantised layers: identical bytes
        assert np.array_equal(ours['weights'][i], ref['weights'][i]) and np.array_equal(ours['biases'][i], ref['biases'][i])
    for i in range(1, L):
        assert np.array_equal(ours['biases'][i], ref['biases'][i])
    # quantised blocks: every value is replaced by its NEAREST codebook entry, and the codebook is at least as good as
    # the reference's (scikit-learn) one on the same data -- the only comparison its unseeded clustering allows
    originals = [g['sd.net_layers.%d.weight' % i].reshape(-1) for i in range(1, L)] + \
                [x[x != 0] for x in (g['sd.feature_grid.%d' % i].reshape(-1) for i in range(ours['header']['n_grids']))]
    for b_ours, b_ref, x in zip(ours['blocks'], ref['blocks'], originals):
        assert b_ours['labels'].size == x.size and np.all(np.diff(b_ours['centres']) >= 0)
        rec = b_ours['centres'][b_ours['labels']]
        nearest = np.abs(x[:, None].astype(np.float64) - b_ours['centres'][None, :].astype(np.float64)).min(1)
        assert np.allclose(np.abs(rec.astype(np.float64) - x), nearest, rtol=0, atol=1e-7 * np.abs(x).max())
        mse_ours = np.mean((rec.astype(np.float64) - x) ** 2)
        mse_ref = np.mean((b_ref['centres'][b_ref['labels']].astype(np.float64) - x) ** 2)
        assert mse_ours <= 1.25 * mse_ref + 1e-12, (mse_ours, mse_ref)
    # our own reader on our own file == the oracle's reading of it, bit for bit
    back = restore_model(path).state_dict()
    for i in range(ours['header']['n_grids']):
        assert np.array_equal(back['feature_grid.%d' % i].cpu().numpy().reshape(-1), ours['grids'][i])
    for i in range(L):
        assert np.array_equal(back['net_layers.%d.weight' % i].cpu().numpy().reshape(-1), ours['weights'][i])


_CARRY_N = 2048 * 1024 + 2049          # 1026 block counts: the scan's second round of 1024 holds two live entries


@pytest.mark.parametrize('density,n', [(d, n) for d in (0.0, 0.3, 1.0)
                                       for n in (1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, 100003, 1 << 20)]
                         + [(0.3, _CARRY_N), (1.0, _CARRY_N)])
def test_mask_compact_expand_bit_exact(dev, n, density):
    from latent_feature_grid_compression_amd import ops
    rng = np.random.default_rng(n + int(density * 10))
    x = rng.standard_normal(n).astype(np.float32)
    x[rng.random(n) >= density] = 0.0
    if density == 1.0:
        x[x == 0] = 1.0
    xt = torch.from_numpy(x).to(dev)
    mask = ops.codec_mask(xt)
    assert np.array_equal(mask.cpu().numpy(), np.packbits((x != 0).astype(np.uint8)))
    nz = ops.codec_compact(xt)
    assert np.array_equal(nz.cpu().numpy(), x[x != 0])
    # expansion from a bit stream in which this tensor starts at an arbitrary (non byte aligned) position
    for off in (0, 5, 8, 13):
        bits = np.concatenate([rng.integers(0, 2, off).astype(np.uint8), (x != 0).astype(np.uint8),
                               rng.integers(0, 2, 11).astype(np.uint8)])
        stream = torch.from_numpy(np.packbits(bits)).to(dev)
        back = ops.codec_expand(stream, off, n, nz)
        assert np.array_equal(back.cpu().numpy(), x), off


@pytest.mark.parametrize('bits', [1, 2, 3, 4, 5, 7, 8, 11, 16])
def test_dequant_matches_reference_bit_slicing(dev, bits):
    from latent_feature_grid_compression_amd import ops
    rng = np.random.default_rng(bits)
    n = 1003
    centres = rng.standard_normal(1 << bits).astype(np.float32)
    stream = rng.integers(0, 256, (n * bits + 7) // 8, dtype=np.uint8)
    labels = K.unpack_labels(stream.tobytes(), n, bits)
    out = ops.codec_dequant(torch.from_numpy(stream).to(dev), bits, n, torch.from_numpy(centres).to(dev))
    assert np.array_equal(out.cpu().numpy(), centres[labels])


def test_kmeans_is_lloyd_from_the_ward_init(dev):
    from latent_feature_grid_compression_amd import ops
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.standard_normal(50000) * 0.1, rng.standard_normal(3000) * 2.0, [7.5, -9.0]]).astype(np.float32)
    rng.shuffle(x)
    k = 256
    centres, labels = ops.codec_kmeans(torch.from_numpy(x).to(dev), k, iterations=25)
    c = centres.cpu().numpy()
    assert np.all(np.diff(c) >= 0)
    # labels: nearest centre (ties at a midpoint may go either way)
    d = np.abs(x[:, None].astype(np.float64) - c[None, :].astype(np.float64))
    lab = labels.cpu().numpy()
    assert np.allclose(d[np.arange(x.size), lab], d.min(1), rtol=0, atol=1e-6)
    # the same Lloyd iteration in numpy (fp64 sums) from the same initial centres (host Ward merge of the sorted values)
    import ctypes
    from latent_feature_grid_compression_amd import _lib
    s = np.sort(x)
    ref = np.empty(k, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    assert _lib.load().lfgc_codec_ward_init_host(s.ctypes.data_as(fp), s.size, k, ref.ctypes.data_as(fp)) == 0
    for _ in range(25):
        mid = 0.5 * (ref[:-1] + ref[1:])
        a = np.searchsorted(mid, x, side='left')
        sums = np.bincount(a, weights=x.astype(np.float64), minlength=k)
        cnt = np.bincount(a, minlength=k)
        ref = np.where(cnt > 0, (sums / np.maximum(cnt, 1)).astype(np.float32), ref)
    assert np.allclose(c, ref, rtol=0, atol=2e-6)
    # fewer values than clusters: still a valid codebook (the reference's scikit-learn call raises here)
    few = torch.tensor([0.5, -1.0, 0.25], device=dev)
    c2, l2 = ops.codec_kmeans(few, 256)
    assert torch.equal(c2[l2.long()], few)


def test_cfg3_sized_round_trip_and_timing(dev, tmp_path):
    """cfg-3 coefficient count (9.6 M, a third pruned): store + restore; structural invariants at full size."""
    import time
    from latent_feature_grid_compression_amd.model.model_utils import setup_model, store_model_parameters, restore_model
    torch.manual_seed(3)
    m = setup_model(3, 128, 1, 4, 'fourier', 2, '', 0.1, 0.9, 'db2', 32, 64, '').to(dev)
    with torch.no_grad():
        for p in m.feature_grid:
            p.mul_((torch.rand_like(p) > 0.33).float())
    path = str(tmp_path / 'cfg3')
    torch.cuda.synchronize(); t0 = time.perf_counter()
    store_model_parameters(m, path)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    back = restore_model(path)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    print('cfg3 codec: store %.3f s, restore %.3f s, file %.1f MB + mask %.1f MB' % (
        t1 - t0, t2 - t1, os.path.getsize(path) / 1e6, os.path.getsize(path + '_mask.bnr') / 1e6))
    for a, b in zip(m.feature_grid, back.feature_grid):
        assert torch.equal(a == 0, b == 0)                                   # pruning pattern survives exactly
        a, b = a.detach(), b.detach()
        nz = a != 0                                                          # 256-entry codebook: error-optimal, so sparse in the tails
        rel_rms = ((a - b)[nz].square().mean().sqrt() / a[nz].square().mean().sqrt()).item()
        rel_max = ((a - b).abs().max() / a.abs().max()).item()
        print('  tensor %s: rms error / rms %.2e, max error / max %.2e' % (tuple(a.shape), rel_rms, rel_max))
        assert rel_rms <= 0.02 and rel_max <= 0.25
        assert torch.unique(b).numel() <= 257
    assert torch.equal(m.net_layers[0].weight, back.net_layers[0].weight)
    assert torch.equal(m.final_layer.bias, back.final_layer.bias)
    n_coef = sum(p.numel() for p in m.feature_grid)
    assert os.path.getsize(path + '_mask.bnr') == (n_coef + 7) // 8


@pytest.mark.parametrize('bits', [4, 8, 12])
def test_restore_reads_other_label_widths(dev, tmp_path, bits):
    """The reader takes the label width from the header (the reference's writer hard-codes 8, its reader does not): a file
    serialised by the oracle with 2^bits-entry codebooks must restore to exactly what the oracle parses from it."""
    from latent_feature_grid_compression_amd.model.model_utils import restore_model
    rng = np.random.default_rng(bits)
    C, G, H, L = 3, 15, 16, 3
    shapes = [(C, 6, 6, 6), (C, 7, 6, 6, 6), (C, 7, 9, 9, 9)]
    grids = [np.where(rng.random(s) > 0.4, rng.standard_normal(s), 0.0).astype(np.float32) for s in shapes]
    k = 1 << bits
    blocks = []
    for n in [H * H] * (L - 1) + [int(np.count_nonzero(g)) for g in grids]:
        blocks.append({'centres': np.sort(rng.standard_normal(k)).astype(np.float32), 'labels': rng.integers(0, k, n)})
    header = dict(n_layers=L, layer_width=H, input_dim=15 + C, input_channel=3, output_dim=1, bit_precision=bits, grid_size=G,
                  n_grids=3, feature_size=C, grid_sizes=[int(np.count_nonzero(g)) for g in grids],
                  zeros=[int(g.size - np.count_nonzero(g)) for g in grids])
    weights = [rng.standard_normal((15 + C) * H).astype(np.float32)] + [None] * (L - 1) + [rng.standard_normal(H).astype(np.float32)]
    biases = [rng.standard_normal(H).astype(np.float32) for _ in range(L)] + [rng.standard_normal(1).astype(np.float32)]
    mask = np.concatenate([(g.reshape(-1) != 0) for g in grids])
    raw, mask_raw = K.serialize(header, weights, biases, blocks, mask)
    path = str(tmp_path / ('bits%d' % bits))
    open(path, 'wb').write(raw)
    open(path + '_mask.bnr', 'wb').write(mask_raw)
    want = K.parse(raw, mask_raw)
    got = restore_model(path).state_dict()
    for i in range(3):
        assert np.array_equal(got['feature_grid.%d' % i].cpu().numpy().reshape(-1), want['grids'][i])
    for i in range(L):
        assert np.array_equal(got['net_layers.%d.weight' % i].cpu().numpy().reshape(-1), want['weights'][i])
        assert np.array_equal(got['net_layers.%d.bias' % i].cpu().numpy(), want['biases'][i])
    assert np.array_equal(got['final_layer.weight'].cpu().numpy().reshape(-1), want['weights'][L])
