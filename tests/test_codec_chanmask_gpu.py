"""GPU tests for the per-cell form of the codec's pruning mask (mode 2 of the mask file): the four
entries bit for bit against the numpy reference (tests/chanmask_ref.py) at the sizes where a selection block of 2048
elements, a wave or a byte boundary can go wrong; the status word of the expansion; and files -- cell-pruned models take
mode 2, equal the reference writer's bytes, are strictly shorter and restore to the same model; dense and
per-coefficient-pruned models keep the ``entropy=True`` file; a mode-2 file whose counts only the device can refute is
refused."""
import functools
import struct

import numpy as np
import pytest
import torch

import chanmask_ref as M
import rans_ref as A
from test_codec_entropy_gpu import files, gpu
from test_codec_entropy_gpu import model as flat_model
from test_hip_forward import dev  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (3, 1), (5, 2047), (5, 2048), (5, 2049), (3, 3375), (32, 4100)]
KINDS = ['mixed', 'ones', 'zeros']


def tensor(C, S, kind, rng):
    """(C, S) fp32.  'mixed': 30 % of the cells alive, a tenth of their entries zero again, a cell alive in one channel only,
    and -0.0 (zero) and NaN (non-zero) entries inside and outside the alive cells."""
    if kind == 'ones':
        return (rng.standard_normal((C, S)).astype(np.float32) + 3.0)
    x = np.zeros((C, S), np.float32)
    if kind == 'mixed':
        alive = rng.random(S) < 0.3
        x[:, alive] = rng.standard_normal((C, int(alive.sum()))).astype(np.float32) + 3.0
        x[rng.random((C, S)) < 0.1] = 0.0
        x[C - 1, S // 2] = 7.0
        x[0, S // 3] = np.nan
    x[rng.random((C, S)) < 0.05] *= -1.0                     # -0.0 among the zeros (and negative values among the rest)
    return x


def bits_of(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def expected(x):
    """(flags, V, out) of the format text for x (C, S)."""
    flags = (x != 0).any(0)
    return flags, x[:, flags], np.where(flags[None, :], x, np.float32(0.0))


# ---- 1. the entries ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C,S', SHAPES)
def test_entries_against_the_reference(dev, C, S):
    from latent_feature_grid_compression_amd import ops
    rng = np.random.default_rng(1000 * C + S)
    for kind in KINDS:
        x = tensor(C, S, kind, rng)
        flags, V, out = expected(x)
        K = int(flags.sum())
        support, residual = M.factor((x != 0).reshape(-1), C)
        assert np.array_equal(support, flags) and (kind != 'ones' or K == S) and (kind != 'zeros' or K == 0)
        xd = gpu(x, dev)
        got_flags = ops.codec_support(xd, C)
        assert got_flags.dtype == torch.uint8 and got_flags.shape == (S,)
        assert np.array_equal(got_flags.cpu().numpy(), flags.astype(np.uint8)), (kind, 'support')
        got_bits = ops.codec_pack_flags(got_flags)
        assert np.array_equal(got_bits.cpu().numpy(), np.packbits(flags)), (kind, 'pack')
        got_V = ops.codec_compact_support(xd, C, got_flags)
        assert got_V.shape == (C, K)
        assert np.array_equal(bits_of(got_V.cpu().numpy()), bits_of(V)), (kind, 'compact')
        if K:
            assert np.array_equal(ops.codec_mask(got_V).cpu().numpy(), np.packbits(residual)), (kind, 'residual')
            nz = ops.codec_compact(got_V).cpu().numpy()                          # the flat tensor's non-zero values, in its order
            assert np.array_equal(bits_of(nz), bits_of(x[x != 0])), (kind, 'values')
        for offset in (0, 3, 13):
            stream = gpu(np.packbits(np.concatenate([np.ones(offset, bool), flags, np.ones(5, bool)])), dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            got = ops.codec_expand_support(stream, offset, C, S, got_V, K, status)
            assert got.shape == (C * S,) and int(status.item()) == 0, (kind, offset)
            assert np.array_equal(bits_of(got.cpu().numpy()), bits_of(out).reshape(-1)), (kind, offset, 'expand')


def test_entries_on_unaligned_buffers(dev):
    """S a multiple of 4 behind a base that is not 16-byte aligned, and flags at an odd address: the scalar paths."""
    from latent_feature_grid_compression_amd import ops
    rng = np.random.default_rng(77)
    C, S = 4, 4096 + 8
    x = tensor(C, S, 'mixed', rng)
    flags, V, out = expected(x)
    shifted = gpu(np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]), dev)[1:]
    assert shifted.data_ptr() % 16 == 4
    got_flags = ops.codec_support(shifted, C)
    assert np.array_equal(got_flags.cpu().numpy(), flags.astype(np.uint8))
    odd = gpu(np.concatenate([np.ones(1, np.uint8), flags.astype(np.uint8) * 255]), dev)[1:]      # any non-zero byte is a flag
    assert odd.data_ptr() % 8 == 1
    assert np.array_equal(ops.codec_pack_flags(odd).cpu().numpy(), np.packbits(flags))
    assert np.array_equal(bits_of(ops.codec_compact_support(shifted, C, odd).cpu().numpy()), bits_of(V))


def test_a_wrong_count_sets_the_status_word(dev):
    from latent_feature_grid_compression_amd import ops
    rng = np.random.default_rng(5)
    C, S = 5, 2049
    x = tensor(C, S, 'mixed', rng)
    flags, V, out = expected(x)
    K = int(flags.sum())
    stream = gpu(np.packbits(flags), dev)
    values = gpu(np.concatenate([V.reshape(-1), np.full(C, 9.0, np.float32)]), dev)         # room for C * (K + 1)
    for k, want in ((K, 0), (K - 1, 1), (K + 1, 1)):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        got = ops.codec_expand_support(stream, 0, C, S, values[:C * k] if k <= K else values, k, status)
        assert int(status.item()) == want, k
        assert np.array_equal(got.cpu().numpy().reshape(C, S)[:, ~flags], out[:, ~flags])   # zeros stay zeros whatever K says
        if k == K:
            assert np.array_equal(bits_of(got.cpu().numpy()), bits_of(out).reshape(-1))
        else:
            with pytest.raises(ValueError, match='other than K'):
                ops.codec_expand_support(stream, 0, C, S, values, k)
    assert ops.codec_expand_support(stream, 0, C, S, values, K).shape == (C * S,)           # checks for itself, and passes
    status = torch.ones(1, dtype=torch.int32, device=dev) * 4                               # accumulated, not overwritten
    ops.codec_expand_support(stream, 0, C, S, values, K - 1, status)
    assert int(status.item()) == 5


# ---- 2. files ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cell_model(which):
    """The 'big' (32^3 x 16 channels, 3 x 128 MLP) and 'small' (15^3 x 3) shapes of test_codec_entropy_gpu.py, Laplace
    coefficients, the 90 % of the cells (over all tensors) with the smallest channel vectors set to zero, and 1 % of the
    coefficients zeroed on top of that."""
    from latent_feature_grid_compression_amd.model.model_utils import setup_model
    torch.manual_seed(9)
    if which == 'big':
        m = setup_model(3, 128, 1, 3, 'fourier', 2, '', 0.1, 0.9, 'db2', 16, 32, '')
    else:
        m = setup_model(3, 16, 1, 3, 'fourier', 2, '', 0.1, 0.9, 'db2', 3, 15, '')
    g = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for p in m.feature_grid:
            u = torch.rand(p.shape, generator=g) - 0.5
            p.copy_(-torch.sign(u) * torch.log1p(-2 * u.abs()))
        norms = torch.cat([p.pow(2).sum(0).reshape(-1) for p in m.feature_grid])
        thr = torch.kthvalue(norms, int(round(0.9 * norms.numel())))[0]
        for p in m.feature_grid:
            p.mul_((p.pow(2).sum(0, keepdim=True) > thr).float())
            p.mul_((torch.rand(p.shape, generator=g) >= 0.01).float())
    return m.to('cuda')


def masks_of(m):
    return [(p.detach().cpu().numpy() != 0).reshape(-1) for p in m.feature_grid]


def store_both(m, tmp_path, bits):
    from latent_feature_grid_compression_amd.model.model_utils import store_model_parameters
    flat_path, cell_path = str(tmp_path / ('flat%d' % bits)), str(tmp_path / ('cell%d' % bits))
    store_model_parameters(m, flat_path, bits, entropy=True)
    store_model_parameters(m, cell_path, bits, entropy=True, channel_mask=True)
    return flat_path, cell_path


def assert_same_model(a, b):
    a, b = a.state_dict(), b.state_dict()
    assert list(a) == list(b)
    for name in a:
        assert a[name].dtype == b[name].dtype and torch.equal(a[name], b[name]), name


@pytest.mark.parametrize('which,bits', [('big', 4), ('big', 8), ('big', 12), ('small', 1), ('small', 4), ('small', 5),
                                        ('small', 8), ('small', 12)])
def test_cell_pruned_model_files(dev, tmp_path, which, bits):
    from latent_feature_grid_compression_amd.model.model_utils import restore_model
    m = cell_model(which)
    C = int(m.feature_grid[0].shape[0])
    flat_path, cell_path = store_both(m, tmp_path, bits)
    flat, cell = files(flat_path), files(cell_path)
    assert cell[0] == flat[0]                                                    # the parameter file: byte for byte
    masks = masks_of(m)
    assert flat[1] == M.flat_mask_file(masks)
    assert cell[1] == M.write_mask_file(masks, C) == M.best_mask_file(masks, C)
    assert cell[1][0] == 2 and len(cell[1]) < len(flat[1])
    print('%s, %2d bits: mask %d -> %d bytes, files %d -> %d bytes' % (which, bits, len(flat[1]), len(cell[1]),
                                                                      sum(map(len, flat)), sum(map(len, cell))))
    back_flat, back_cell = restore_model(flat_path), restore_model(cell_path)
    assert_same_model(back_flat, back_cell)
    for p, q in zip(m.feature_grid, back_cell.feature_grid):
        assert torch.equal(p == 0, q == 0)


@pytest.mark.parametrize('keep', [1.0, 0.1])
def test_dense_and_per_coefficient_pruned_models_keep_the_flat_file(dev, tmp_path, keep):
    from latent_feature_grid_compression_amd.model.model_utils import restore_model
    m = flat_model('big', keep)
    C = int(m.feature_grid[0].shape[0])
    flat_path, cell_path = store_both(m, tmp_path, 8)
    flat, cell = files(flat_path), files(cell_path)
    assert cell == flat
    masks = masks_of(m)
    assert cell[1] == M.best_mask_file(masks, C) and cell[1][0] == 1
    assert not len(M.write_mask_file(masks, C)) < len(flat[1])                  # mode 2 loses the size comparison
    assert_same_model(restore_model(flat_path), restore_model(cell_path))


def tampered_pair(tmp_path, kind):
    """A mode-2 pair every host check accepts and only the device can refute.  'K': the last tensor's K one too small, the
    residual field shortened to match; 'residual': one residual bit more than the tensor has non-zero coefficients."""
    m = cell_model('big')
    C = int(m.feature_grid[0].shape[0])
    _, path = store_both(m, tmp_path, 8)
    parts = [M.factor(mask, C) for mask in masks_of(m)]
    K = [int(s.sum()) for s, _ in parts]
    support = np.concatenate([s for s, _ in parts])
    residual = np.concatenate([r for _, r in parts])
    nz = int(parts[-1][1].sum())
    if kind == 'K':
        assert nz <= C * (K[-1] - 1)                                             # still host-valid
        K[-1] -= 1
        residual = residual[:-C]
    else:
        residual = residual.copy()
        residual[np.flatnonzero(~residual)[-1]] = True                           # a zero inside a kept cell of the last tensor
    with open(path + '_mask.bnr', 'wb') as f:
        f.write(bytes([2]) + b''.join(struct.pack('<I', k) for k in K) + M.field(support) + M.field(residual))
    return path


@pytest.mark.parametrize('kind', ['K', 'residual'])
def test_counts_only_the_device_can_refute(dev, tmp_path, kind):
    from latent_feature_grid_compression_amd.model.model_utils import restore_model
    with pytest.raises(ValueError, match='does not hold the number of set bits'):
        restore_model(tampered_pair(tmp_path, kind))
