"""Host tests of the error-bounded residual layer: the numpy reference (tests/residual_ref.py) obeys
its own guarantee on adversarial inputs, the file parser accepts the reference writer's bytes and refuses every malformed
file before any device call (no GPU here proves that), and the argument checks of the public entry."""
import struct

import numpy as np
import pytest
import torch

import residual_ref as RR

EPS = [1e-1, 1e-3, 1e-6]


# ---- 1. the reference against its own guarantee ----------------------------------------------------------------------------------

@pytest.mark.parametrize('eps', EPS)
def test_reference_obeys_its_guarantee_on_adversarial_inputs(eps):
    for p, g in (RR.adversarial(eps), RR.mixture(4100, eps, 5), RR.mixture(7, eps, 2)):
        sym = RR.quantise(p, g, eps)
        out = RR.apply(p, sym, eps, RR.outliers(sym, g))
        bad = RR.violations(out, g, eps)
        assert bad.size == 0, (eps, bad[:5], p[bad[:5]], g[bad[:5]])
        assert sym.dtype == np.uint8 and sym.shape == p.shape


@pytest.mark.parametrize('eps', EPS)
def test_reference_on_each_adversarial_kind(eps):
    p, g = RR.adversarial(eps)
    sym, first, second = RR.quantise(p, g, eps, detail=True)
    e32, step, inv = RR.steps(eps)
    with np.errstate(all='ignore'):
        t = (g - p) * inv
        ties = np.isfinite(t) & (np.abs(t - np.floor(t)) == 0.5) & (np.abs(t) < 100)
    assert ties.sum() >= 3                                                    # exact half-step ties are among the inputs ...
    kept = ties & (sym != RR.ESCAPE)                                          # (one that escapes did so through the bound test)
    assert np.all(second[ties & ~kept]) and kept.sum() >= 2            # t = +-0.5 always stays: r = p, |g - p| = eps
    q = (sym[kept].astype(np.int32) >> 1) ^ -(sym[kept].astype(np.int32) & 1)
    assert np.all(q % 2 == 0)                                                 # ... and they round to even
    same = np.isfinite(p) & (p == g)
    assert same.sum() >= 7 and np.all(sym[same] == 0)                         # g == p and the four signed-zero pairs
    nonfinite = ~np.isfinite(p) | ~np.isfinite(g)
    assert nonfinite.sum() == 8 and np.all(sym[nonfinite] == RR.ESCAPE) and np.all(first[nonfinite])
    far = np.isfinite(t) & (np.abs(t) > 1e5)
    assert far.sum() == 2 and np.all(first[far])                              # 1e6 steps: out of the symbol range
    edge = np.isfinite(t) & (np.abs(np.abs(t) - 127.5) < 0.01)                # 127.5 steps: q = 127 or 128 by the rounding of t;
    assert edge.sum() == 2 and np.all(first[edge] | (np.abs(np.rint(t[edge])) == 127))      # either way the guarantee test above holds
    near = np.isfinite(t) & (np.abs(np.abs(t) - 126.5) < 0.01)
    assert near.sum() == 2 and not first[near].any()                          # 126.5 steps: in range (bound decides)
    esc = RR.outliers(sym, g)
    assert esc.size == int((sym == RR.ESCAPE).sum())
    assert esc.view(np.uint32)[-1] == 0x7FC12345                              # verbatim: the NaN payload survives


def test_second_escape_test_triggers_at_small_eps():
    """eps = 1e-6 with values near 1: r is rounded to 1.2e-7, so voxels whose exact residual lies within 6e-8 of the bound
    break it after rounding; only the second test catches them."""
    p, g = RR.mixture(20000, 1e-6, 3)
    sym, first, second = RR.quantise(p, g, 1e-6, detail=True)
    assert second.sum() >= 1, 'no voxel escaped through the bound test: the case is not covered'
    assert np.all(sym[second] == RR.ESCAPE) and not (first & second).any()
    # without the second test those voxels would break the guarantee
    s = sym.astype(np.int32)
    s[second] = 0
    e32, step, inv = RR.steps(1e-6)
    t = (g[second] - p[second]) * inv
    r = p[second] + np.rint(t).astype(np.float32) * step
    assert np.all(np.abs(g[second].astype(np.float64) - r.astype(np.float64)) > np.float64(e32))


def test_checksum_is_order_free_and_sensitive():
    rng = np.random.default_rng(0)
    p = rng.standard_normal(1000).astype(np.float32)
    bits = p.view(np.uint32).astype(object)
    want = sum(int(b) * (2 * i + 1) for i, b in enumerate(bits)) % (1 << 64)
    assert RR.checksum(p) == want
    q = p.copy()
    q.view(np.uint32)[517] ^= 1
    assert RR.checksum(q) != want
    q = p.copy()
    q[[3, 4]] = q[[4, 3]]
    assert RR.checksum(q) != want                                             # position-weighted: a swap shows


# ---- 2. the file parser --------------------------------------------------------------------------------------------------------------

def volume(seed=1, shape=(5, 6, 7)):
    rng = np.random.default_rng(seed)
    pred = rng.uniform(-1, 1, shape).astype(np.float32)
    gt = (pred + rng.normal(0, 0.05, shape)).astype(np.float32)
    gt[1, 2, 3] = np.float32('nan')
    gt[4, 0, 0] = pred[4, 0, 0] + 10.0
    return pred, gt


def test_parser_accepts_the_reference_writers_bytes():
    from latent_feature_grid_compression_amd.model.residual_codec import parse_residual_file
    pred, gt = volume()
    for slab_planes, eps in ((2, 1e-2), (5, 1e-2), (1, 1e-3), (5, 10.0)):
        raw, modes = RR.write_file(pred, gt, eps, 8, slab_planes)
        info = parse_residual_file(raw)
        ref = RR.read_file(raw)
        assert (info.X, info.Y, info.Z, info.tiled_res, info.slab_planes) == (5, 6, 7, 8, slab_planes)
        assert np.float32(info.eps) == np.float32(eps)
        assert len(info.records) == len(ref['records']) == -(-5 // slab_planes)
        for rec, want, mode in zip(info.records, ref['records'], modes):
            assert (rec.x0, rec.x1, rec.K, rec.checksum, rec.mode) == (want['x0'], want['x1'], want['K'], want['checksum'], mode)
            assert rec.n == (rec.x1 - rec.x0) * 42
            at, nbytes = rec.payload
            assert rec.outliers == at + nbytes
            if mode == 1:
                assert rec.rans.n == rec.n and rec.rans.nbytes == nbytes
            else:
                assert rec.rans is None and nbytes == rec.n
            assert np.array_equal(np.frombuffer(raw, '<f4', rec.K, rec.outliers).view(np.uint32), want['outliers'].view(np.uint32))
        back = RR.restore(raw, pred)
        assert RR.violations(back, gt, eps).size == 0 and back.view(np.uint32)[1, 2, 3] == gt.view(np.uint32)[1, 2, 3]
    big, modes = RR.write_file(np.zeros((40, 10, 10), np.float32), np.zeros((40, 10, 10), np.float32), 1e-2, 32, 40)
    assert modes == [1] and parse_residual_file(big).records[0].mode == 1     # 4000 zero symbols: the stream is shorter


def patched(raw, offset, fmt, *values):
    b = bytearray(raw)
    struct.pack_into(fmt, b, offset, *values)
    return bytes(b)


def malformed_files():
    pred, gt = volume()
    raw, _ = RR.write_file(pred, gt, 1e-2, 8, 2)                              # three records, every one mode 0 (84 symbols)
    coded, modes = RR.write_file(np.zeros((40, 10, 10), np.float32), np.zeros((40, 10, 10), np.float32), 1e-2, 32, 40)
    assert modes == [1]
    first = RR.HEADER.size                                                     # offset of the first record
    cases = {
        'bad magic': patched(raw, 0, '<4s', b'LFGX'),
        'bad version': patched(raw, 4, '<B', 2),
        'reserved byte set': patched(raw, 6, '<B', 1),
        'zero X': patched(raw, 8, '<I', 0),
        'zero Y': patched(raw, 12, '<I', 0),
        'zero Z': patched(raw, 16, '<I', 0),
        'eps zero': patched(raw, 20, '<f', 0.0),
        'eps negative': patched(raw, 20, '<f', -1e-2),
        'eps nan': patched(raw, 20, '<f', float('nan')),
        'eps inf': patched(raw, 20, '<f', float('inf')),
        'tiled_res zero': patched(raw, 24, '<I', 0),
        'slab_planes zero': patched(raw, 28, '<I', 0),
        'header cut': raw[:31],
        'record head cut': raw[:first + 5],
        'payload cut': raw[:first + RR.RECORD.size + 40],
        'outliers cut': raw[:-2],
        'last record missing': raw[:first + (len(raw) - first) // 3],
        'K above the voxel count': patched(raw, first, '<I', 85),
        'unknown mode': patched(raw, first + 12, '<B', 2),
        'trailing bytes': raw + b'\x00',
        'stream of another symbol count': patched(coded, first + RR.RECORD.size, '<I', 3999),
        'stream cut': coded[:-1],
        'stream then trailing bytes': coded + b'\x00\x00',
    }
    return cases


@pytest.mark.parametrize('name', sorted(malformed_files()))
def test_parser_refuses_malformed_files(name):
    from latent_feature_grid_compression_amd.model.residual_codec import parse_residual_file
    with pytest.raises(ValueError):
        parse_residual_file(malformed_files()[name])


def test_restore_refuses_a_malformed_file_before_any_device_call(tmp_path):
    from latent_feature_grid_compression_amd.model.model_utils import restore_volume
    path = str(tmp_path / 'bad.lfgr')
    with open(path, 'wb') as f:
        f.write(malformed_files()['trailing bytes'])
    with pytest.raises(ValueError, match='trailing'):
        restore_volume(None, None, path)                                      # neither dataset nor model is looked at


# ---- 3. argument checks -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('bad', [0, 0.0, -1e-3, float('nan'), float('inf'), 1e-50, 1e39, 3e38, 'tight', None])
def test_store_residuals_refuses_a_bad_max_error(bad, tmp_path):
    from latent_feature_grid_compression_amd.model.model_utils import store_residuals
    path = tmp_path / 'never.lfgr'
    with pytest.raises(ValueError, match='max_error'):
        store_residuals(None, None, None, str(path), bad)                     # refused before anything else is looked at
    assert not path.exists()


def test_store_residuals_refuses_bad_shapes_and_steps():
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    from latent_feature_grid_compression_amd.model.residual_codec import store_residuals
    ds = IndexDataset((4, 5, 6), build_index_table=False)
    good = torch.zeros(4, 5, 6)
    for kwargs in (dict(tiled_res=0), dict(tiled_res=2.5), dict(slab_planes=0), dict(slab_planes=-1)):
        with pytest.raises(ValueError):
            store_residuals(ds, None, good, 'never.lfgr', 1e-3, **kwargs)
    for gt in (torch.zeros(4, 5, 7), torch.zeros(4, 5, 6, dtype=torch.float64), np.zeros((4, 5, 6), np.float32)):
        with pytest.raises(ValueError, match='gt_vol'):
            store_residuals(ds, None, gt, 'never.lfgr', 1e-3)


def test_ops_wrappers_check_dtypes_and_shapes_on_the_host():
    from latent_feature_grid_compression_amd import ops
    f, d, u = torch.zeros(8), torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.uint8)
    for call in (lambda: ops.residual_quantize(d, f, 1e-3), lambda: ops.residual_quantize(f, d, 1e-3),
                 lambda: ops.residual_quantize(f, torch.zeros(9), 1e-3), lambda: ops.residual_quantize(f, f, 0.0),
                 lambda: ops.residual_quantize(torch.zeros(8, 2)[:, 0], f, 1e-3),
                 lambda: ops.residual_outliers(f, f), lambda: ops.residual_outliers(u, torch.zeros(9)),
                 lambda: ops.residual_apply(f, f, 1e-3, f[:0]), lambda: ops.residual_apply(f, u[:7], 1e-3, f[:0]),
                 lambda: ops.residual_apply(f, u, 1e-3, torch.zeros(9)), lambda: ops.residual_apply(f, u, -1.0, f[:0]),
                 lambda: ops.residual_apply(f, u, 1e-3, d[:0])):
        with pytest.raises(ValueError):
            call()
    assert ops.residual_eps(np.float32(1e-3)) == float(np.float32(1e-3))


def test_c_entries_refuse_bad_arguments_before_any_launch():
    """Every call below fails a host-side check of the entry (a negative code: nothing was launched), so the made-up
    addresses are never touched and no device is needed."""
    from latent_feature_grid_compression_amd import _lib
    lib = _lib.load()
    a, big = 1 << 20, 1 << 30                                                  # a non-null, 16-byte aligned address; a workspace size
    quantize = lambda pred=a, gt=a, n=8, eps=1e-3, sym=a, cks=a: lib.lfgc_residual_quantize_f32(pred, gt, n, eps, sym, cks, None)
    outliers = lambda sym=a, gt=a, n=8, out=a, count=a, ws=a, nbytes=big: lib.lfgc_residual_outliers_f32(sym, gt, n, out, count, ws,
                                                                                                          nbytes, None)
    apply = lambda pred=a, sym=a, n=8, eps=1e-3, esc=a, K=1, out=a, cks=a, ne=a, st=a, ws=a, nbytes=big: \
        lib.lfgc_residual_apply_f32(pred, sym, n, eps, esc, K, out, cks, ne, st, ws, nbytes, None)
    E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -4, -5
    for eps in (0.0, -1e-3, float('nan'), float('inf'), 1e-45, 1e-39, 3e38):   # zero, negative, NaN, Inf, denormal, step = Inf
        assert quantize(eps=eps) == E_SHAPE and apply(eps=eps) == E_SHAPE, eps
    assert quantize(eps=8e37) == E_SHAPE                                      # 1 / step is denormal
    assert quantize(n=0) == E_SHAPE and outliers(n=0) == E_SHAPE and apply(n=0) == E_SHAPE
    assert apply(K=9) == E_SHAPE and apply(K=-1) == E_SHAPE
    assert quantize(pred=None) == E_NULL and quantize(gt=None) == E_NULL and quantize(sym=None) == E_NULL and quantize(cks=None) == E_NULL
    assert outliers(sym=None) == E_NULL and outliers(count=None) == E_NULL and outliers(ws=None) == E_NULL
    assert apply(esc=None, K=1) == E_NULL and apply(out=None) == E_NULL and apply(st=None) == E_NULL and apply(ne=None) == E_NULL
    assert quantize(pred=a + 2) == E_ALIGN and quantize(gt=a + 1) == E_ALIGN and quantize(cks=a + 4) == E_ALIGN
    assert outliers(gt=a + 2) == E_ALIGN and outliers(count=a + 4) == E_ALIGN
    assert apply(out=a + 2) == E_ALIGN and apply(esc=a + 1) == E_ALIGN and apply(ne=a + 4) == E_ALIGN and apply(st=a + 2) == E_ALIGN
    assert outliers(nbytes=0) == E_WORKSPACE and apply(nbytes=0) == E_WORKSPACE
    for n in (1, 2048, 2049, 10 ** 7):
        need = lib.lfgc_residual_workspace_bytes(n)
        assert need == lib.lfgc_codec_select_workspace_bytes(n) > 0
        assert outliers(n=n, nbytes=need - 1) == E_WORKSPACE and apply(n=n, nbytes=need - 1) == E_WORKSPACE
