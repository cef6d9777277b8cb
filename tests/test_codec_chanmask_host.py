"""CPU tests for the per-cell form of the codec's pruning mask (mode 2 of the mask file): the numpy
reference (tests/chanmask_ref.py) against itself, the size premise on the CPU, the premise that the project's own pruning
code zeroes whole cells, ``restore_model``'s host checks of a mode-2 pair (all made before anything touches the GPU), the
writer's argument check, and the four new C entries: declared, bound, exported, and validating their arguments."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest
import torch

import chanmask_ref as M
import rans_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_WORKSPACE = -1, -2, -5
ONE = ctypes.c_void_p(16)                 # any non-NULL aligned address: nothing is launched, nothing dereferenced on these paths
NEW_SYMBOLS = ['lfgc_codec_support_f32', 'lfgc_codec_pack_flags_u8', 'lfgc_codec_compact_support_f32',
               'lfgc_codec_expand_support_f32']
PATTERNS = ['cell-shared', 'per-coefficient', 'all ones', 'one channel zero', 'one channel only']


def pattern(kind, C, S, rng):
    """A flat mask (C * S,) bool."""
    if kind == 'cell-shared':                               # 10 % of the cells, a few exact zeros inside them
        m = np.broadcast_to(rng.random(S) < 0.1, (C, S)) & ~(rng.random((C, S)) < 0.01)
    elif kind == 'per-coefficient':
        m = rng.random((C, S)) < 0.1
    elif kind == 'all ones':
        m = np.ones((C, S), bool)
    elif kind == 'one channel zero':
        m = np.broadcast_to(rng.random(S) < 0.3, (C, S)).copy()
        m[C // 2] = False
    else:
        assert kind == 'one channel only'                   # a cell that is non-zero in one channel only, among shared cells
        m = np.broadcast_to(rng.random(S) < 0.1, (C, S)).copy()
        m[:, S // 2] = False
        m[C - 1, S // 2] = True
    return np.ascontiguousarray(m).reshape(-1)


# ---- 1. the reference -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [1, 3, 8, 32])
def test_reference_round_trips(C):
    rng = np.random.default_rng(50 + C)
    for kind in PATTERNS:
        sizes = (1, 13, 70, 3375)                            # none a multiple of 8
        masks = [pattern(kind, C, S, rng) for S in sizes]
        for m, S in zip(masks, sizes):
            support, residual = M.factor(m, C)
            assert support.shape == (S,) and residual.shape == (C * int(support.sum()),)
            assert np.array_equal(support, m.reshape(C, S).any(0))
            assert np.array_equal(residual[residual], m[m])  # the set residual bits are the set mask bits, in order
            assert int(residual.sum()) == int(m.sum())
            assert np.array_equal(M.unfactor(support, residual, C), m), (kind, C, S)
        buf = M.write_mask_file(masks, C)
        assert buf[0] == 2
        back, K, modes = M.parse_mask_file(buf, [m.size for m in masks], C)
        assert K == [int(m.reshape(C, -1).any(0).sum()) for m in masks]
        for a, b in zip(masks, back):
            assert np.array_equal(a, b), (kind, C)
        if kind == 'all ones':
            assert K == list(sizes)


def test_reference_bit_positions():
    """The format text, by hand: C = 2, two tensors of 3 and 2 cells."""
    x0 = np.array([[1, 0, 0], [1, 0, 1]], bool)              # support 1 0 1, K = 2, residual (c-major) 1 0 | 1 1
    x1 = np.array([[0, 0], [0, 1]], bool)                    # support 0 1,   K = 1, residual 0 | 1
    buf = M.write_mask_file([x0.reshape(-1), x1.reshape(-1)], 2)
    assert buf == bytes([2]) + struct.pack('<II', 2, 1) + bytes([0, 0b10101000]) + bytes([0, 0b10110100])


# ---- 2. the size premise ------------------------------------------------------------------------------------------------------

def test_size_premise():
    """C = 16, S = 32 768, 10 % of the cells kept, 1 % further zeros inside them: the per-cell file is far below the flat one;
    for a per-coefficient mask of the same density it is not, and the writer keeps the flat file."""
    C, S, keep = 16, 32768, 0.1
    rng = np.random.default_rng(0)
    shared = (np.broadcast_to(rng.random(S) < keep, (C, S)) & ~(rng.random((C, S)) < 0.01)).reshape(-1)
    iid = (rng.random((C, S)) < keep * 0.99).reshape(-1)
    sizes = {name: (len(M.write_mask_file([m], C)), len(M.flat_mask_file([m]))) for name, m in (('shared', shared), ('iid', iid))}
    print('mode 2 / flat bytes:', sizes)
    assert M.flat_mask_file([shared])[0] == 1 and M.flat_mask_file([iid])[0] == 1
    assert sizes['shared'][0] < sizes['shared'][1]
    assert 5 * sizes['shared'][0] < sizes['shared'][1]                            # 3 919 against 31 595
    assert not sizes['iid'][0] < sizes['iid'][1]                                  # 33 003 against 31 569
    assert M.best_mask_file([shared], C)[0] == 2 and M.best_mask_file([iid], C)[0] == 1


# ---- 3. the premise from the project's own pruning code -----------------------------------------------------------------------------

def test_pruning_layers_zero_whole_cells():
    """Smallify layers are built per cell (size = f.shape[1:]): after save_dropvalues_on_grid and remove_drop_layers every
    tensor's zero pattern is the same in all channels, and it is the chosen per-cell mask."""
    from latent_feature_grid_compression_amd.model.model_utils import setup_model
    torch.manual_seed(3)
    m = setup_model(3, 16, 1, 3, 'fourier', 2, 'smallify', 0.1, 0.75, 'db2', 5, 12, '')
    g = torch.Generator().manual_seed(4)
    chosen = []
    with torch.no_grad():
        for p, d in zip(m.feature_grid, m.drop):
            assert tuple(d.betas.shape) == tuple(p.shape[1:])
            p.copy_(torch.rand(p.shape, generator=g) + 0.5)                       # no accidental zeros
            d.betas.copy_(torch.rand(d.betas.shape, generator=g) + 0.5)
            keep = torch.rand(d.betas.shape, generator=g) < 0.3
            d.tracker.EMAVar = torch.where(keep, 0.0, 1.0)                        # pruned where the variance exceeds the threshold
            chosen.append(keep)
    m.save_dropvalues_on_grid('cpu')
    m.remove_drop_layers('cpu')
    assert len(m.feature_grid) == len(chosen) >= 2
    for p, keep in zip(m.feature_grid, chosen):
        nz = p.detach() != 0
        assert nz.any() and not nz.all()
        assert torch.equal(nz, keep.unsqueeze(0).expand_as(nz))
        C = p.shape[0]
        support, residual = M.factor(nz.numpy().reshape(-1), C)
        assert residual.all() and residual.size == C * int(keep.sum())            # the residual has nothing left to say


# ---- 4. restore_model's checks, on files the reference writers made ------------------------------------------------------------------

BITS, WIDTH, C = 4, 64, 2
TOTAL = 65536
CELLS = TOTAL // C


def reference_files():
    """An entropy-mode parameter file and its mode-2 mask file (support field in mode 1): one coefficient tensor of 32 768
    cells x 2 channels, 10 % of the cells kept, a few zeros inside."""
    rng = np.random.default_rng(22)
    mask = (np.broadcast_to(rng.random(CELLS) < 0.1, (C, CELLS)) & ~(rng.random((C, CELLS)) < 0.02)).reshape(-1)
    nz = int(mask.sum())
    header = dict(n_layers=2, layer_width=WIDTH, input_dim=15 + C, input_channel=3, output_dim=1, bit_precision=BITS,
                  grid_size=16, n_grids=1, feature_size=C, grid_sizes=[nz], zeros=[TOTAL - nz])
    weights = [rng.standard_normal((15 + C) * WIDTH).astype(np.float32), None, rng.standard_normal(WIDTH).astype(np.float32)]
    biases = [rng.standard_normal(WIDTH).astype(np.float32)] * 2 + [np.zeros(1, np.float32)]
    blocks = [{'centres': np.arange(16, dtype=np.float32), 'labels': rng.integers(0, 16, WIDTH * WIDTH)},
              {'centres': np.arange(16, dtype=np.float32) - 8, 'labels': rng.integers(0, 16, nz)}]
    param, _, _ = A.write_files(header, weights, biases, blocks, mask)
    mask_file = M.write_mask_file([mask], C)
    K = int(mask.reshape(C, CELLS).any(0).sum())
    assert mask_file[0] == 2 and struct.unpack_from('<I', mask_file, 1)[0] == K and mask_file[5] == 1
    return param, mask_file, nz, K


def restore(tmp_path, param, mask_file):
    from latent_feature_grid_compression_amd.model.model_utils import restore_model
    path = str(tmp_path / 'model')
    open(path, 'wb').write(param)
    open(path + '_mask.bnr', 'wb').write(mask_file)
    return restore_model(path)


def no_device(*a, **k):
    raise AssertionError('restore_model reached the device before refusing the file')


def test_reference_mode2_files_parse_back_and_pass_the_host_checks(tmp_path, monkeypatch):
    param, mask_file, nz, K = reference_files()
    masks, Ks, modes = M.parse_mask_file(mask_file, [TOTAL], C)
    assert Ks == [K] and int(masks[0].sum()) == nz and modes[0] == 1
    assert np.array_equal(masks[0], A.parse_files(param, M.flat_mask_file(masks))['mask'])
    monkeypatch.setattr(torch.Tensor, 'to', no_device)
    monkeypatch.setattr(torch.Tensor, 'cuda', no_device)
    with pytest.raises(AssertionError, match='reached the device'):            # so the refusals below are not vacuous
        restore(tmp_path, param, mask_file)


BAD_MODE2_KINDS = ['truncated', 'truncated counts', 'trailing bytes', 'support field mode', 'residual field mode', 'channels',
                   'K above S', 'K too small', 'symbol count', 'stream word count']


def bad_mode2_pair(kind):
    """reference_files() with one thing wrong (tests/test_codec_container_host.py parses these directly)."""
    param, mask_file, nz, K = reference_files()
    param, mask_file = bytearray(param), bytearray(mask_file)
    support_at = 1 + 4                                                           # the support field's mode byte
    residual_at = support_at + 1 + A.stream_info(bytes(mask_file), support_at + 1)['nbytes']
    assert mask_file[residual_at] in (0, 1)
    if kind == 'truncated':
        mask_file = mask_file[:-2]
    elif kind == 'truncated counts':
        mask_file = mask_file[:3]
    elif kind == 'trailing bytes':
        mask_file += b'\x00'
    elif kind == 'support field mode':
        mask_file[support_at] = 2
    elif kind == 'residual field mode':
        mask_file[residual_at] = 2
    elif kind == 'channels':                                                     # 65 536 coefficients are no multiple of 3
        param[8] = 3
    elif kind == 'K above S':
        struct.pack_into('<I', mask_file, 1, CELLS + 1)
    elif kind == 'K too small':                                                  # grid_sizes[0] > C * K
        assert nz > C * (nz // C - 1)
        struct.pack_into('<I', mask_file, 1, nz // C - 1)
    elif kind == 'symbol count':                                                 # the support stream names 4097 symbols
        assert struct.unpack_from('<I', mask_file, support_at + 1)[0] == CELLS // 8
        struct.pack_into('<I', mask_file, support_at + 1, CELLS // 8 + 1)
    elif kind == 'stream word count':
        w0 = struct.unpack_from('<I', mask_file, support_at + 1 + A.HEADER)[0]
        struct.pack_into('<I', mask_file, support_at + 1 + A.HEADER, w0 + 1)
    return bytes(param), bytes(mask_file)


@pytest.mark.parametrize('kind', BAD_MODE2_KINDS)
def test_restore_model_refuses_a_bad_mode2_pair_before_any_device_use(tmp_path, monkeypatch, kind):
    param, mask_file = bad_mode2_pair(kind)
    monkeypatch.setattr(torch.Tensor, 'to', no_device)
    monkeypatch.setattr(torch.Tensor, 'cuda', no_device)
    with pytest.raises(ValueError):
        restore(tmp_path, param, mask_file)


# ---- 5. the writer's argument check ------------------------------------------------------------------------------------------------------

def test_channel_mask_needs_entropy(tmp_path):
    from latent_feature_grid_compression_amd.model import model_utils as MU
    m = MU.setup_model(3, 16, 1, 3, 'fourier', 2, '', 0.1, 0.9, 'db2', 3, 15, '')          # on the CPU: refused before any device use
    for kwargs in ({'channel_mask': True}, {'entropy': False, 'channel_mask': True}):
        with pytest.raises(ValueError, match='entropy=True'):
            MU.store_model_parameters(m, str(tmp_path / 'x'), 8, **kwargs)
    assert not os.path.exists(str(tmp_path / 'x'))


def test_writer_keeps_the_strictly_smallest_mode(tmp_path, monkeypatch):
    """Host stand-ins for the device steps: the per-cell file is taken only where it is strictly smaller than the flat one."""
    from latent_feature_grid_compression_amd.model import model_utils as MU
    m = MU.setup_model(3, 16, 1, 3, 'fourier', 2, '', 0.1, 0.9, 'db2', 3, 15, '')
    monkeypatch.setattr(MU, '_device_flat', lambda t: t.detach().float().reshape(-1))
    monkeypatch.setattr(MU, '_quantised_block', lambda values, bits, entropy=False: b'B' * 5)
    monkeypatch.setattr(MU.ops, 'codec_compact', lambda g: g[g != 0])
    monkeypatch.setattr(MU.ops, 'codec_mask', lambda g: torch.from_numpy(np.packbits((g != 0).numpy())))
    monkeypatch.setattr(MU.ops, 'codec_rans_encode', lambda s: torch.zeros(10 ** 9, dtype=torch.uint8, device='meta'))
    total = sum(p.numel() for p in m.feature_grid)
    flat_len = 1 + (total + 7) // 8                                              # mode 0: the stand-in stream never wins
    for per_cell_len, want in ((flat_len - 1, 2), (flat_len, 0), (flat_len + 1, 0)):
        monkeypatch.setattr(MU, '_channel_mask_file', lambda grids, channels, n=per_cell_len: b'\x02' * n)
        path = str(tmp_path / ('m%d' % per_cell_len))
        MU.store_model_parameters(m, path, 8, entropy=True, channel_mask=True)
        got = open(path + '_mask.bnr', 'rb').read()
        assert got[0] == want and len(got) == min(per_cell_len, flat_len)
    MU.store_model_parameters(m, path, 8, entropy=True)                          # without the option mode 2 is not even formed
    assert open(path + '_mask.bnr', 'rb').read()[0] == 0


# ---- 6. the library -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def lib():
    from latent_feature_grid_compression_amd import _lib
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    from latent_feature_grid_compression_amd import _lib, ops
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lfgc.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(lfgc_[a-z0-9_]+)\s*\(', header))
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
    for fn in ('codec_support', 'codec_pack_flags', 'codec_compact_support', 'codec_expand_support'):
        assert callable(getattr(ops, fn))


def test_counted_expansion_reads_the_total_where_the_selection_leaves_it():
    """ops.codec_expand(..., counted=True) indexes the workspace by the selection's workgroup size: the two must agree."""
    from latent_feature_grid_compression_amd import ops
    text = open(os.path.join(ROOT, 'latent_feature_grid_compression_amd', 'csrc', 'lfgc_select.h')).read()
    block = int(re.search(r'constexpr int kSelectBlock = (\d+);', text).group(1))
    passes = int(re.search(r'constexpr int kSelectPasses = (\d+);', text).group(1))
    assert 'kSelectPerBlock = kSelectBlock * kSelectPasses' in text and ops._SELECT_PER_BLOCK == block * passes == 2048
    assert 'offsets[nblocks] takes the' in text                                  # the total's place, as lfgc_select.h states it


def test_entries_validate_their_arguments_on_the_host(lib):
    """include/lfgc.h's return codes, decided before anything is launched: no device is touched and no pointer read."""
    ws = lib.lfgc_codec_select_workspace_bytes(5000)
    assert lib.lfgc_codec_support_f32(None, 3, 10, ONE, None) == E_NULL
    assert lib.lfgc_codec_support_f32(ONE, 3, 10, None, None) == E_NULL
    for Cc, S in ((0, 10), (3, 0), (-1, 10), (3, -5), (4, 1 << 62)):
        assert lib.lfgc_codec_support_f32(ONE, Cc, S, ONE, None) == E_SHAPE
        assert lib.lfgc_codec_compact_support_f32(ONE, Cc, S, ONE, ONE, ONE, ONE, 1 << 20, None) == E_SHAPE
        assert lib.lfgc_codec_expand_support_f32(ONE, 0, Cc, S, ONE, 0, ONE, ONE, ONE, 1 << 20, None) == E_SHAPE
    assert lib.lfgc_codec_pack_flags_u8(None, 10, ONE, None) == E_NULL
    assert lib.lfgc_codec_pack_flags_u8(ONE, 10, None, None) == E_NULL
    assert lib.lfgc_codec_pack_flags_u8(ONE, 0, ONE, None) == E_SHAPE
    for missing in range(5):
        args = [ONE] * 5
        args[missing] = None
        x, flags, V, count, wsp = args
        assert lib.lfgc_codec_compact_support_f32(x, 3, 5000, flags, V, count, wsp, ws, None) == E_NULL
        support, V, out, status, wsp = args
        assert lib.lfgc_codec_expand_support_f32(support, 0, 3, 5000, V, 7, out, status, wsp, ws, None) == E_NULL
    assert lib.lfgc_codec_compact_support_f32(ONE, 3, 5000, ONE, ONE, ONE, ONE, ws - 1, None) == E_WORKSPACE
    assert lib.lfgc_codec_expand_support_f32(ONE, 0, 3, 5000, ONE, 7, ONE, ONE, ONE, ws - 1, None) == E_WORKSPACE
    assert lib.lfgc_codec_expand_support_f32(ONE, -1, 3, 5000, ONE, 7, ONE, ONE, ONE, ws, None) == E_SHAPE
    assert lib.lfgc_codec_expand_support_f32(ONE, 0, 3, 5000, ONE, -1, ONE, ONE, ONE, ws, None) == E_SHAPE
    assert lib.lfgc_codec_expand_support_f32(ONE, 0, 3, 5000, ONE, 5001, ONE, ONE, ONE, ws, None) == E_SHAPE


def test_wrappers_check_their_arguments_before_the_device():
    from latent_feature_grid_compression_amd import _lib, ops
    with pytest.raises(ValueError):
        ops.codec_support(torch.zeros(10), 3)                                    # 10 is no multiple of 3
    with pytest.raises(ValueError):
        ops.codec_pack_flags(torch.zeros(8))                                     # not bytes
    with pytest.raises(_lib.LfgcError):
        ops.codec_support(torch.zeros(12), 3)                                    # valid, so only then asks for the GPU
    with pytest.raises(_lib.LfgcError):
        ops.codec_pack_flags(torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(_lib.LfgcError):
        ops.codec_compact_support(torch.zeros(12), 3, torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(_lib.LfgcError):
        ops.codec_expand_support(torch.zeros(1, dtype=torch.uint8), 0, 3, 4, torch.zeros(6), 2)
