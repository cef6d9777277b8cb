"""GPU tests of the error-bounded residual layer: the three entries bit for bit against the numpy
reference (tests/residual_ref.py) at every size where the 4-wide path, a wave or a selection block of 2048 can go wrong, on
aligned bases and on views offset by one element; the guarantee itself in float64 on every voxel, independently of the
reference; the status path with too few outliers; store_residuals / restore_volume end to end over a small model; and a
changed model reported as PredictionMismatch."""
import copy
import functools
import struct
import warnings

import numpy as np
import pytest
import torch

import residual_ref as RR
from test_hip_forward import dev  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 63, 64, 65, 2047, 2048, 2049, 4100]
EPS = [1e-1, 1e-3, 1e-6]
U64 = (1 << 64) - 1


def on_device(a, offset):
    """A device copy of a 1-D array: on an aligned base, or the view [1:] of a buffer one element longer."""
    a = np.asarray(a)
    if not offset:
        return torch.from_numpy(a.copy()).cuda()
    buf = torch.zeros(a.size + 1, dtype=torch.from_numpy(a[:0].copy()).dtype, device='cuda')
    buf[1:] = torch.from_numpy(a.copy()).cuda()
    return buf[1:]


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.reshape(-1).view(np.uint32)


@functools.lru_cache(maxsize=None)
def entries(eps, offset):
    """Every size once through the three entries: what the device gave, as host arrays, next to the inputs."""
    from latent_feature_grid_compression_amd import ops
    runs = []
    for n in SIZES:
        p, g = RR.mixture(n, eps, 100 + n)
        pred, gt = on_device(p, offset), on_device(g, offset)
        sym_buf = on_device(np.zeros(n, np.uint8), offset)
        assert (pred.data_ptr() % 16 == 0) == (not offset) and (sym_buf.data_ptr() % 4 == 0) == (not offset)
        sym, cks = ops.residual_quantize(pred, gt, eps, sym=sym_buf)
        assert sym.data_ptr() == sym_buf.data_ptr()
        esc = ops.residual_outliers(sym, gt)
        out, cks2, n_escape, status = ops.residual_apply(pred, sym, eps, esc)
        alias = on_device(p, offset)
        same, cks3, n_escape3, status3 = ops.residual_apply(alias, sym, eps, esc, out=alias)
        assert same.data_ptr() == alias.data_ptr() and out.data_ptr() != pred.data_ptr()
        assert np.array_equal(bits(pred), bits(p)) and np.array_equal(bits(gt), bits(g))      # the inputs were left alone
        runs.append(dict(n=n, p=p, g=g, sym=sym.cpu().numpy(), checksum=int(cks.item()) & U64, outliers=esc.cpu().numpy(),
                         out=out.cpu().numpy(), checksum_apply=int(cks2.item()) & U64, n_escape=int(n_escape.item()),
                         status=int(status.item()), alias=same.cpu().numpy(), checksum_alias=int(cks3.item()) & U64,
                         n_escape_alias=int(n_escape3.item()), status_alias=int(status3.item())))
    return runs


# ---- 1. the entries against the reference, bit for bit ----------------------------------------------------------------------------

@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'offset'])
@pytest.mark.parametrize('eps', EPS)
def test_entries_equal_the_reference_bit_for_bit(dev, eps, offset):
    seen_escape = seen_second = False
    for r in entries(eps, offset):
        tag = (eps, offset, r['n'])
        want, first, second = RR.quantise(r['p'], r['g'], eps, detail=True)
        assert np.array_equal(r['sym'], want), (tag, np.flatnonzero(r['sym'] != want)[:8])
        assert r['checksum'] == RR.checksum(r['p']), tag
        esc = RR.outliers(want, r['g'])
        assert np.array_equal(bits(r['outliers']), bits(esc)), tag
        restored = RR.apply(r['p'], want, eps, esc)
        assert np.array_equal(bits(r['out']), bits(restored)), (tag, np.flatnonzero(bits(r['out']) != bits(restored))[:8])
        assert np.array_equal(bits(r['alias']), bits(restored)), tag          # out aliasing pred gives the same bits
        for k in ('checksum_apply', 'checksum_alias'):
            assert r[k] == r['checksum'], (tag, k)
        assert r['n_escape'] == r['n_escape_alias'] == esc.size and r['status'] == r['status_alias'] == 0, tag
        seen_escape |= bool(esc.size)
        seen_second |= bool(second.any())
    assert seen_escape and (seen_second or eps > 1e-6)                        # the cases did reach the escape paths


# ---- 2. the guarantee, independently of the reference ------------------------------------------------------------------------------

@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'offset'])
@pytest.mark.parametrize('eps', EPS)
def test_guarantee_holds_at_every_voxel(dev, eps, offset):
    bound = np.float64(np.float32(eps))
    for r in entries(eps, offset):
        g = r['g']
        for out in (r['out'], r['alias']):
            fin = np.isfinite(g)
            err = np.abs(out[fin].astype(np.float64) - g[fin].astype(np.float64))
            assert np.all(err <= bound), (eps, offset, r['n'], float(err.max()))
            assert np.array_equal(bits(out[~fin]), bits(g[~fin])), (eps, offset, r['n'])


# ---- 3. the status path ----------------------------------------------------------------------------------------------------------------

def test_too_few_outliers_are_reported_and_never_read_past(dev):
    from latent_feature_grid_compression_amd import ops
    eps = 1e-3
    p, g = RR.mixture(4100, eps, 77)
    sym = RR.quantise(p, g, eps)
    esc = RR.outliers(sym, g)
    E = esc.size
    assert E >= 3 and np.flatnonzero(sym == RR.ESCAPE).max() > 2048           # escapes in more than one selection block
    want = RR.apply(p, sym, eps, esc)
    where = np.flatnonzero(sym == RR.ESCAPE)
    pred, s = torch.from_numpy(p).cuda(), torch.from_numpy(sym).cuda()
    short = torch.from_numpy(esc[:E - 1].copy()).cuda()                       # sized exactly: E - 1 floats
    out, _, n_escape, status = ops.residual_apply(pred, s, eps, short)
    assert int(n_escape.item()) == E and int(status.item()) & 2 and int(status.item()) & 1
    got = out.cpu().numpy()
    keep = np.ones(p.size, bool)
    keep[where[-1]] = False
    assert np.array_equal(bits(got[keep]), bits(want[keep])) and bits(got)[where[-1]] == 0
    none = torch.empty(0, dtype=torch.float32, device='cuda')                 # K = 0: no outlier is there to be read
    out, _, n_escape, status = ops.residual_apply(pred, s, eps, none)
    assert int(n_escape.item()) == E and int(status.item()) == 3
    got = out.cpu().numpy()
    assert np.all(bits(got)[where] == 0)
    keep[where] = False
    assert np.array_equal(bits(got[keep]), bits(want[keep]))
    full, _, n_escape, status = ops.residual_apply(pred, s, eps, torch.from_numpy(esc).cuda())
    assert int(status.item()) == 0 and int(n_escape.item()) == E and np.array_equal(bits(full), bits(want))


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------

RES = (20, 17, 13)                                                            # no multiple of either tile


@functools.lru_cache(maxsize=None)
def scene():
    """(dataset, model in eval mode, ground truth on the host): the small model of the entropy tests over a smooth synthetic
    volume plus noise."""
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    from test_codec_entropy_gpu import model
    m = copy.deepcopy(model('small', 1.0)).eval()
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, r) for r in RES], indexing='ij')
    rng = np.random.default_rng(4)
    gt = 0.6 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y) * np.cos(1.3 * z - 0.2) + 0.02 * rng.standard_normal(RES)
    return IndexDataset(RES, build_index_table=False), m, torch.from_numpy(gt.astype(np.float32))


def prediction(ds, m, tiled_res, slab_planes):
    """The device's own prediction, slab by slab as the encoder launches it."""
    from latent_feature_grid_compression_amd.visualization.OutputToVTK import field_from_net_fused
    return np.concatenate([field_from_net_fused(ds, m, x0, x1, tiled_res).cpu().numpy() for x0, x1 in RR.slabs(RES[0], slab_planes)])


def assert_bound(out, gt, eps):
    err = np.abs(out.astype(np.float64) - gt.astype(np.float64))
    assert np.all(err <= np.float64(np.float32(eps))), float(err.max())


@pytest.mark.parametrize('tiled_res', [8, 32])
@pytest.mark.parametrize('slab_planes', [1, 7, None])
def test_store_and_restore(dev, tmp_path, slab_planes, tiled_res):
    from latent_feature_grid_compression_amd.model.model_utils import parse_residual_file, restore_volume, store_residuals
    ds, m, gt = scene()
    g = gt.numpy()
    path = str(tmp_path / 'vol.lfgr')
    planes = RES[0] if slab_planes is None else slab_planes                   # the default takes the whole small volume
    pred = prediction(ds, m, tiled_res, planes)
    n_slab = planes * RES[1] * RES[2]

    # a bound inside the residual's range: the bound at every voxel, and the reference writer's bytes
    eps = 1e-2
    stats = store_residuals(ds, m, gt if tiled_res == 8 else gt.cuda(), path, eps, tiled_res, slab_planes)
    raw = open(path, 'rb').read()
    info = parse_residual_file(raw)
    assert (info.tiled_res, info.slab_planes, len(info.records)) == (tiled_res, planes, -(-RES[0] // planes))
    want, _ = RR.write_file(pred, g, eps, tiled_res, planes)
    assert len(raw) == len(want) and raw == want
    assert stats['bytes'] == len(raw) and stats['escapes'] == sum(r.K for r in info.records)
    assert stats['bits_per_voxel'] == 8.0 * len(raw) / g.size
    out = restore_volume(ds, m, path)
    assert out.is_cuda and tuple(out.shape) == RES and out.dtype == torch.float32
    assert_bound(out.cpu().numpy(), g, eps)
    assert np.array_equal(bits(out), bits(RR.restore(raw, pred)))
    given = torch.full(RES, 7.0, device='cuda')
    assert restore_volume(ds, m, path, out=given) is given and torch.equal(given, out)

    # a bound above max |g - p|: every symbol 0.  A record takes mode 1 where its all-zero stream (8 + 512 bytes of header,
    # 4 + 256 per chunk of 32 768 symbols, no words) is strictly shorter than its symbols -- a slab of one plane has 221
    # symbols, which no stream undercuts: there the record keeps mode 0, as the format's rule says.
    eps = float(np.float32(1.01 * np.abs(g.astype(np.float64) - pred).max()))
    stats = store_residuals(ds, m, gt, path, eps, tiled_res, slab_planes)
    raw = open(path, 'rb').read()
    info = parse_residual_file(raw)
    ref = RR.read_file(raw)
    assert stats['escapes'] == 0 and all(not r['sym'].any() and r['K'] == 0 for r in ref['records'])
    stream = 520 + 260 * -(-n_slab // 32768)
    if stream < n_slab:
        assert all(r.mode == 1 for r in info.records)
        assert len(raw) < len(RR.write_file(pred, g, eps, tiled_res, planes, force_mode=0)[0])
    else:
        assert all(r.mode == 0 for r in info.records)
    assert raw == RR.write_file(pred, g, eps, tiled_res, planes)[0]
    out = restore_volume(ds, m, path).cpu().numpy()
    assert np.array_equal(bits(out), bits(pred))                              # nothing to add: the prediction itself
    assert_bound(out, g, eps)

    # a bound far below the residual: nearly every voxel escapes and comes back exactly
    eps = 1e-7
    stats = store_residuals(ds, m, gt, path, eps, tiled_res, slab_planes)
    ref = RR.read_file(open(path, 'rb').read())
    escaped = np.concatenate([r['sym'] == RR.ESCAPE for r in ref['records']])
    assert stats['escapes'] == int(escaped.sum()) > g.size // 2
    out = restore_volume(ds, m, path).cpu().numpy()
    assert np.array_equal(bits(out.reshape(-1)[escaped]), bits(g.reshape(-1)[escaped]))
    assert_bound(out, g, eps)


# ---- 5. a prediction that is not the encoder's ----------------------------------------------------------------------------------------

def test_changed_model_is_a_prediction_mismatch(dev, tmp_path):
    from latent_feature_grid_compression_amd.model.model_utils import PredictionMismatch, parse_residual_file, restore_volume, \
        store_residuals
    ds, m, gt = scene()
    path = str(tmp_path / 'vol.lfgr')
    store_residuals(ds, m, gt, path, 1e-3, 8, 7)
    raw = open(path, 'rb').read()
    changed = copy.deepcopy(m)
    with torch.no_grad():
        changed.net_layers[1].weight[3, 5] += 0.25
    assert issubclass(PredictionMismatch, ValueError)
    with pytest.raises(PredictionMismatch):
        restore_volume(ds, changed, path)
    with pytest.warns(UserWarning, match='bound does not hold'):
        out = restore_volume(ds, changed, path, strict=False)
    assert out.is_cuda and tuple(out.shape) == RES
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        restore_volume(ds, m, path)                                           # the encoder's model: no warning, no error

    # one record's K lowered by one, its last outlier dropped so that the file still parses: the symbols hold more escapes
    rec = next(r for r in parse_residual_file(raw).records if r.K >= 1)
    head = rec.payload[0] - RR.RECORD.size
    end = rec.outliers + 4 * rec.K
    lowered = raw[:head] + struct.pack('<I', rec.K - 1) + raw[head + 4:end - 4] + raw[end:]
    assert parse_residual_file(lowered).records[0].K >= 0                     # the host checks pass
    bad = str(tmp_path / 'lowered.lfgr')
    with open(bad, 'wb') as f:
        f.write(lowered)
    with pytest.raises(ValueError, match='escapes') as info:
        restore_volume(ds, m, bad)
    assert not isinstance(info.value, PredictionMismatch)
    plain = raw[:head] + struct.pack('<I', rec.K - 1) + raw[head + 4:]        # K lowered and nothing else: the layout breaks
    with open(bad, 'wb') as f:
        f.write(plain)
    with pytest.raises(ValueError):
        restore_volume(ds, m, bad)
