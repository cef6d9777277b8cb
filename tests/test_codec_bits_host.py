"""CPU tests for the codec's label widths 1 to 16: the writer's ``bit_precision`` check fires before any device use, and the
new C-ABI entry points (label packer, sorted k-means, uint16 labels) report NULL / shape errors before anything is launched."""
import ctypes

import pytest
import torch

E_NULL, E_SHAPE = -1, -2
ONE = ctypes.c_void_p(16)                 # any non-NULL address: nothing is launched, nothing dereferenced on these paths


@pytest.fixture(scope='module')
def lib():
    from latent_feature_grid_compression_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('bad', [0, 17, -1, 8.5])
def test_store_refuses_a_bad_bit_precision_before_any_device_use(tmp_path, bad):
    from latent_feature_grid_compression_amd.model.model_utils import setup_model, store_model_parameters
    m = setup_model(3, 16, 1, 3, 'fourier', 2, '', 0.1, 0.9, 'db2', 3, 15, '')          # on the CPU
    path = tmp_path / 'never_written'
    with pytest.raises(ValueError, match='bit_precision'):
        store_model_parameters(m, str(path), bit_precision=bad)
    assert not path.exists()


def test_pack_labels_argument_errors(lib):
    assert lib.lfgc_codec_pack_labels(None, 1, 8, 4, ONE, 4, None) == E_NULL
    assert lib.lfgc_codec_pack_labels(ONE, 1, 8, 4, None, 4, None) == E_NULL
    for bits in (0, 17):
        assert lib.lfgc_codec_pack_labels(ONE, 2, 8, bits, ONE, 64, None) == E_SHAPE
    assert lib.lfgc_codec_pack_labels(ONE, 1, 8, 9, ONE, 64, None) == E_SHAPE            # uint8 labels cannot hold 9 bits
    assert lib.lfgc_codec_pack_labels(ONE, 3, 8, 4, ONE, 64, None) == E_SHAPE            # label_bytes is 1 or 2
    assert lib.lfgc_codec_pack_labels(ONE, 1, 0, 4, ONE, 64, None) == E_SHAPE
    assert lib.lfgc_codec_pack_labels(ONE, 1, 9, 3, ONE, 3, None) == E_SHAPE             # 27 bits need 4 bytes
    assert lib.lfgc_codec_pack_labels(ONE, 2, 1 << 28, 16, ONE, (1 << 29) - 1, None) == E_SHAPE   # n * bits = 2^32: 64-bit


def test_sorted_kmeans_argument_errors(lib):
    ws = lib.lfgc_codec_kmeans_sorted_workspace_bytes(5000, 65536)
    assert ws >= 8 * (5 + 65537)                                  # fp64 block sums of 1 024 values + k + 1 int64 bounds
    assert lib.lfgc_codec_kmeans1d_sorted_f32(None, 10, 512, ONE, 1, ONE, 1 << 20, None) == E_NULL
    assert lib.lfgc_codec_kmeans1d_sorted_f32(ONE, 10, 512, None, 1, ONE, 1 << 20, None) == E_NULL
    assert lib.lfgc_codec_kmeans1d_sorted_f32(ONE, 10, 512, ONE, 1, None, 1 << 20, None) == E_NULL
    for k in (0, 65537):
        assert lib.lfgc_codec_kmeans_sorted_workspace_bytes(10, k) == 0
        assert lib.lfgc_codec_kmeans1d_sorted_f32(ONE, 10, k, ONE, 1, ONE, 1 << 20, None) == E_SHAPE
    assert lib.lfgc_codec_kmeans1d_sorted_f32(ONE, 0, 512, ONE, 1, ONE, 1 << 20, None) == E_SHAPE
    assert lib.lfgc_codec_kmeans1d_sorted_f32(ONE, 10, 512, ONE, -1, ONE, 1 << 20, None) == E_SHAPE
    assert lib.lfgc_codec_kmeans1d_sorted_f32(ONE, 5000, 65536, ONE, 1, ONE, ws - 1, None) == -5   # LFGC_E_WORKSPACE
    # the 8-bit entry is as it was
    assert lib.lfgc_codec_kmeans1d_f32(ONE, 10, 257, ONE, ONE, 1, ONE, 1 << 20, None) == E_SHAPE


def test_labels_u16_argument_errors(lib):
    assert lib.lfgc_codec_labels_u16_f32(None, 10, 512, ONE, ONE, None) == E_NULL
    assert lib.lfgc_codec_labels_u16_f32(ONE, 10, 512, None, ONE, None) == E_NULL
    assert lib.lfgc_codec_labels_u16_f32(ONE, 10, 512, ONE, None, None) == E_NULL
    for k in (0, 65537):
        assert lib.lfgc_codec_labels_u16_f32(ONE, 10, k, ONE, ONE, None) == E_SHAPE
    assert lib.lfgc_codec_labels_u16_f32(ONE, 0, 512, ONE, ONE, None) == E_SHAPE


def test_ops_refuse_host_tensors_and_bad_widths():
    from latent_feature_grid_compression_amd import _lib, ops
    with pytest.raises(_lib.LfgcError):
        ops.codec_pack_labels(torch.zeros(8, dtype=torch.uint8), 4)
    with pytest.raises(_lib.LfgcError):
        ops.codec_kmeans(torch.zeros(8), 512)
