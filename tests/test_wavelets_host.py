"""CPU tests of the wavelet bases beyond db2 (Haar and other 2- to 8-tap banks): filter buffers against the
reference-captured ones, the QMF relations of the built-in banks, the oracle's encode / decode with the captured
filters against the reference's round trips, the level counts, the host-side encode, and the new C-ABI symbols."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
LENGTHS = (2, 6, 8)
NEW_SYMBOLS = ('lfgc_idwt_level_len_f32', 'lfgc_idwt_level_bwd_len_f32', 'lfgc_idwt_level_cl_len_f32',
               'lfgc_idwt_level_cl_bwd_len_f32', 'lfgc_idwt_level_drop_len_f32', 'lfgc_idwt_level_drop_bwd_len_f32',
               'lfgc_dwt_level_len_f32')


def _twt():
    from latent_feature_grid_compression_amd.wavelet_transform import Torch_Wavelet_Transform
    return Torch_Wavelet_Transform


def _ops():
    from latent_feature_grid_compression_amd import ops
    return ops


class Bank:
    """A pywt.Wavelet-like object: anything with a ``filter_bank``."""

    def __init__(self, bank):
        self.filter_bank = tuple(tuple(float(v) for v in row) for row in bank)


@pytest.fixture(scope='module')
def filters():
    return np.load(os.path.join(GOLD, 'wavelets_filters.npz'))


def _wavelet(filters, L):
    return 'haar' if L == 2 else Bank(filters['bank_%d' % L])


@pytest.mark.parametrize('name', ['haar', 'db1'])
def test_haar_buffers_bit_equal_reference(filters, name):
    f = _twt().WaveletFilter3d(name)
    assert f.filter_length == 2
    assert torch.equal(f.filter_fwd, torch.from_numpy(filters['filter_fwd_2']))
    assert torch.equal(f.filter_rev, torch.from_numpy(filters['filter_rev_2']))
    assert set(dict(f.state_dict())) == {'filter_fwd', 'filter_rev'}


@pytest.mark.parametrize('L', [6, 8])
def test_bank_object_buffers_bit_equal_reference(filters, L):
    f = _twt().WaveletFilter3d(Bank(filters['bank_%d' % L]))
    assert f.filter_length == L
    assert torch.equal(f.filter_fwd, torch.from_numpy(filters['filter_fwd_%d' % L]))
    assert torch.equal(f.filter_rev, torch.from_numpy(filters['filter_rev_%d' % L]))


@pytest.mark.parametrize('table', ['_HAAR', '_DB2'])
def test_builtin_banks_follow_qmf_relations(table):
    """dec_lo = reversed rec_lo, rec_hi[k] = (-1)^k rec_lo[L-1-k], dec_hi = reversed rec_hi (PyWavelets' relations)."""
    dec_lo, dec_hi, rec_lo, rec_hi = (list(r) for r in getattr(_twt(), table))
    L = len(rec_lo)
    assert dec_lo == rec_lo[::-1]
    assert rec_hi == [(-1) ** k * rec_lo[L - 1 - k] for k in range(L)]
    assert dec_hi == rec_hi[::-1]


def test_haar_bank_values():
    s = 0.7071067811865476
    assert [list(r) for r in _twt()._HAAR] == [[s, s], [-s, s], [s, s], [s, -s]]


def test_odd_and_long_filters_refused():
    WaveletFilter3d = _twt().WaveletFilter3d
    with pytest.raises(NotImplementedError, match=r'\[ERROR\] Implementation does not support uneven filter length'):
        WaveletFilter3d(Bank([[0.1, 0.2, 0.3]] * 4))
    with pytest.raises(NotImplementedError):
        WaveletFilter3d(Bank([[0.1] * 10] * 4))


@pytest.mark.parametrize('L', LENGTHS)
def test_separable_bank_roundtrip(filters, L):
    """filter_taps' factoring finds a 1-D bank of every captured (8,L,L,L) buffer (taps within an ulp or two: the
    outer product reproduces the buffer to 4e-7 of its largest tap, exactly for the Haar bank)."""
    ops = _ops()
    for key in ('filter_fwd_%d' % L, 'filter_rev_%d' % L):
        f3d = filters[key]
        bank = ops._factor_bank(f3d)
        assert bank is not None and bank.shape == (2, L)
        err = np.abs(ops._outer_bank(bank) - f3d.reshape(8, L, L, L)).max()
        assert err <= 4e-7 * np.abs(f3d).max()
        if L == 2:
            assert err == 0.0


def test_level_counts():
    ops, dwt_max_level = _ops(), _twt().dwt_max_level
    with open(os.path.join(GOLD, 'wavelets_levels.json')) as f:
        table = json.load(f)
    assert table['L2_G64']['num_levels'] == 6 and table['L2_G64']['shape_array'][0] == [2, 2, 2]
    for key, ent in table.items():
        L, G = (int(v) for v in key[1:].split('_G'))
        assert dwt_max_level(G, L) == R.dwt_max_level(G, L) == ent['num_levels'], key
        if ent['num_levels'] == 0:
            continue
        # coefficient shapes: each level d = dwt_out_shape(n, L) of the finer one
        shapes = [tuple(s) for s in ent['shape_array']][::-1]
        dims = [tuple(c[-3:]) for c in ent['coeff_shapes']][1:][::-1]
        for n, d in zip(shapes, dims):
            assert tuple(ops.dwt_out_shape(n, L)) == d, (key, n, d)
        assert tuple(ent['coeff_shapes'][0][-3:]) == dims[-1]


@pytest.mark.parametrize('L', LENGTHS)
def test_oracle_roundtrip_bit_equal_reference(filters, L):
    z = np.load(os.path.join(GOLD, 'wavelets_roundtrip_L%d.npz' % L))
    ffwd, frev = torch.from_numpy(filters['filter_fwd_%d' % L]), torch.from_numpy(filters['filter_rev_%d' % L])
    for G in (15, 16, 17):
        grid = torch.from_numpy(z['G%d.input' % G])
        coeffs, shape_array = R.encode_volume(grid, ffwd)
        assert np.array_equal(shape_array, z['G%d.shape_array' % G])
        assert len(coeffs) == int(z['G%d.n' % G])
        for i, c in enumerate(coeffs):
            assert torch.equal(c, torch.from_numpy(z['G%d.coeff%d' % (G, i)])), (G, i)
        assert torch.equal(R.decode_volume(coeffs, shape_array, frev), torch.from_numpy(z['G%d.decoded' % G]))
    coeffs, shape = R.wavelet_encode(torch.from_numpy(z['nc_input']), ffwd)
    assert torch.equal(coeffs, torch.from_numpy(z['nc_coeffs']))
    assert np.array_equal(shape, z['nc_shape'])
    assert torch.equal(R.wavelet_decode(coeffs, shape, frev), torch.from_numpy(z['nc_decoded']))


@pytest.mark.parametrize('L', LENGTHS)
def test_host_encode_matches_reference(filters, L):
    """The module's host-side (CPU tensor) encode, used while a model is built on the host."""
    z = np.load(os.path.join(GOLD, 'wavelets_roundtrip_L%d.npz' % L))
    f = _twt().WaveletFilter3d(_wavelet(filters, L))
    coeffs, shape = f.encode(torch.from_numpy(z['nc_input']))
    assert torch.equal(coeffs, torch.from_numpy(z['nc_coeffs']))
    assert np.array_equal(shape, z['nc_shape'])


def test_haar_model_builds_on_host():
    from latent_feature_grid_compression_amd.model.Feature_Grid_Model import Feature_Grid_Model
    from latent_feature_grid_compression_amd.model.Feature_Embedding import FourierEmbedding
    z = np.load(os.path.join(GOLD, 'wavelets_haar_model.npz'))
    C, G = int(z['meta'][0]), int(z['meta'][1])
    m = Feature_Grid_Model(FourierEmbedding(2, 3), torch.zeros(C, G, G, G), None, _twt().WaveletFilter3d('haar'),
                           hidden_channel=int(z['meta'][2]), num_layer=int(z['meta'][3]))
    assert np.array_equal(np.asarray(m.shape_array), z['shape_array'])
    sd = m.state_dict()
    assert [k for k in sd] == [k[3:] for k in z.files if k.startswith('sd.')]
    for k, v in sd.items():
        assert tuple(v.shape) == z['sd.' + k].shape, k


def test_new_symbols_exported():
    from latent_feature_grid_compression_amd import _lib
    from latent_feature_grid_compression_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    header = open(os.path.join(ROOT, 'include', 'lfgc.h')).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + '(' in header, name
