"""GPU tests of the renderer's empty-space skipping: the three kernels against the NumPy restatement (tests/skip_ref.py)
for EQUALITY -- ranges and occupancy are exact, the skip loop restates every fp32 operation --, the ground-truth render
with skipping against the one without, bit for bit, and the network render with skipping against code that skips nothing
but is told which blocks are empty."""
import numpy as np
import pytest
import torch

import render_ref as RR
import skip_ref as SR
from test_hip_forward import build_synth, dev  # noqa: F401
from test_render_gpu import _ops, _render, _t

pytestmark = pytest.mark.gpu

F = np.float32


# ---- 1. brick ranges --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('res,B', [((2, 2, 2), 8), ((9, 9, 9), 8), ((10, 9, 17), 8), ((5, 6, 7), 2), ((33, 9, 34), 4),
                                   ((3, 3, 130), 8), ((3, 4, 600), 300)])
def test_brick_minmax_equals_the_restatement(dev, res, B):
    ops = _ops()
    rng = np.random.default_rng(sum(res) + B)
    for planted in (False, True):
        vol = rng.normal(size=res).astype(F)
        if planted:                                                # one NaN, two +inf, two -inf
            at = rng.choice(vol.size, 5, replace=False)
            vol.reshape(-1)[at] = [np.nan, np.inf, np.inf, -np.inf, -np.inf]
        _check_minmax(dev, vol, B)
    assert tuple(ops.brick_table(res, B, dev).shape) == SR.brick_minmax(vol, B).shape


def _check_minmax(dev, vol, B):
    ops = _ops()
    res = vol.shape
    want = SR.brick_minmax(vol, B)
    nb = want.shape[:3]
    n_bricks = int(np.prod(nb))
    dvol = _t(vol, dev)
    for planes in (res[0], 1, 2, 5):
        buf = torch.empty((n_bricks + 1, 2), dtype=torch.float32, device=dev)
        buf[:, 0], buf[:, 1] = float('inf'), float('-inf')
        buf[n_bricks] = torch.tensor([12345.0, -54321.0], device=dev)              # the sentinel row after the table
        table = buf[:n_bricks].view(*nb, 2)
        for xb in range(0, res[0], planes):
            xe = min(xb + planes, res[0])
            ops.brick_minmax(dvol[xb:xe].contiguous(), res, xb, xe, B, table)
        got = buf.cpu().numpy()
        assert np.array_equal(got[:n_bricks].reshape(want.shape), want), (res, B, planes)
        assert got[n_bricks].tolist() == [12345.0, -54321.0]


def test_a_slab_touches_only_the_bricks_that_hold_its_planes(dev):
    ops = _ops()
    res, B = (20, 5, 5), 4                                         # x bricks 0..4 hold the planes 0-4, 4-8, 8-12, 12-16, 16-19
    vol = torch.zeros(res, device=dev)
    for xb, xe, bricks in [(4, 5, [0, 1]), (5, 8, [1]), (7, 13, [1, 2, 3]), (19, 20, [4]), (16, 17, [3, 4]), (0, 1, [0])]:
        table = ops.brick_table(res, B, dev)
        ops.brick_minmax(vol[xb:xe].contiguous(), res, xb, xe, B, table)
        hit = torch.isfinite(table[:, 0, 0, 0]).cpu().numpy()
        assert np.nonzero(hit)[0].tolist() == bricks, (xb, xe)


# ---- 2. occupancy -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('margin', [0.0, 1e-5])
@pytest.mark.parametrize('ext', [(0, 5), (5, 0), (0, 0, 0, 4, 8), (3, 0, 0, 0, 2), (0, 0, 1, 0, 0, 0, 2, 0, 0), (0,) * 9])
def test_brick_occupancy_equals_the_restatement(dev, ext, margin):
    ops = _ops()
    K = len(ext)
    rng = np.random.default_rng(K)
    table = np.concatenate([rng.uniform(0, 1, (K, 3)), np.array(ext, np.float64)[:, None]], 1).astype(F)
    v_min, v_max = -1.0, 1.0
    nodes = np.linspace(v_min, v_max, K).astype(F)
    lo = rng.uniform(-1.5, 1.5, 2000).astype(F)
    hi = (lo + rng.uniform(0, 1, 2000).astype(F) ** 3).astype(F)
    hi[:200] = lo[:200]                                            # points
    lo[200:500] = rng.choice(nodes, 300)                           # ranges that begin ...
    hi[400:800] = rng.choice(nodes, 400)                           # ... and end exactly on nodes (some both)
    hi = np.maximum(lo, hi)
    hi[800:900] = np.nextafter(hi[800:900], F(np.inf))             # and an ulp past them
    lo[900:950], hi[900:950] = -np.inf, np.inf                     # bricks that hold a NaN
    lo[950:975] = -np.inf
    hi[975:1000] = np.inf
    mm = np.stack([lo, hi], 1).reshape(10, 20, 10, 2)
    want = SR.occupancy(mm, table, v_min, v_max, margin)
    got = ops.brick_occupancy(_t(mm, dev), _t(table, dev), v_min, v_max, margin)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (10, 20, 10)
    assert np.array_equal(got.cpu().numpy(), want)
    if any(ext) and not all(ext):
        assert 0 < want.sum() < want.size
    else:
        assert want.sum() == (want.size if all(ext) else 0)


# ---- 3. the skip kernel -----------------------------------------------------------------------------------------------------

_CELLS, _B = (21, 13, 9), 4                                        # bricks (6, 4, 3), the last ones of 1 cell
_DT = 0.0123                                                       # a third of RR.DT: up to 220 steps, several blocks of 64


def _skip_rays():
    o, d = RR.ray_set()
    rn, rf, rs = RR.clip(o, d, RR.BOX[0], RR.BOX[1], 0.0, np.inf, _DT, RR.ray_max_steps(_DT))
    return o, d, rn, rf, rs


def _occupancy_pattern(name):
    nb = SR.brick_counts(_CELLS, _B)
    rng = np.random.default_rng(len(name))
    occ = np.zeros(nb, np.uint8)
    if name == 'full':
        occ[:] = 1
    elif name == 'random':
        occ = (rng.uniform(size=nb) < 0.3).astype(np.uint8)
    elif name == 'one':
        occ[3, 2, 1] = 1
    return occ


@pytest.mark.parametrize('pattern', ['empty', 'full', 'random', 'one'])
@pytest.mark.parametrize('k0', [0, 1])
@pytest.mark.parametrize('S', [32, 64])
def test_ray_skip_equals_the_restatement(dev, S, k0, pattern):
    ops = _ops()
    o, d, rn, rf, rs = _skip_rays()
    R_ = o.shape[0]
    rs = rs.copy()
    hits = np.nonzero(rs > 0)[0]
    rs[hits[5::40]] = 1                                            # 1-step rays
    k_next = np.full(R_, k0 * S, np.int32)
    k_next[hits[7::40]] = rs[hits[7::40]]                          # rays at ...
    k_next[hits[9::40]] = rs[hits[9::40]] + 3 * S                  # ... and past their end
    occ = _occupancy_pattern(pattern)
    od, dd, tn, tf, n = (_t(a, dev) for a in (o, d, rn, rf, rs))
    docc = _t(occ, dev)
    assert (rs > 64).sum() > 10 and (rs == 0).sum() > 10

    def run(live):
        k = _t(k_next, dev)
        skipped = torch.zeros(R_, dtype=torch.int32, device=dev)
        ops.ray_skip(None if live is None else _t(live, dev), od, dd, tn, tf, n, k, _DT, S, RR.BOX[0], RR.BOX[1], _CELLS, _B,
                     docc, skipped)
        return k.cpu().numpy(), skipped.cpu().numpy()

    # every ray (live = NULL), misses included
    want_k, want_s = SR.skip(range(R_), o, d, rn, rf, rs, k_next, _DT, S, RR.BOX[0], RR.BOX[1], _CELLS, _B, occ)
    got_k, got_s = run(None)
    assert np.array_equal(got_k, want_k) and np.array_equal(got_s, want_s)
    started = k_next < rs
    if pattern == 'empty':
        assert (got_k[started] >= rs[started]).all() and (got_s[started] > 0).all()
    if pattern == 'full':
        assert np.array_equal(got_k, k_next) and not got_s.any()
    if pattern in ('random', 'one'):                  # some rays jump, some stop in front of a brick
        assert (got_s[started] > 0).any() and (got_k[started] < rs[started]).any()
    assert np.array_equal(got_k[~started], k_next[~started]) and not got_s[~started].any()
    assert ((got_k - k_next) == got_s * S).all()
    # a sub-list (no multiple of 8 rays: the last workgroup is partly filled): rays outside it are untouched
    sub = np.ascontiguousarray(np.arange(R_, dtype=np.int32)[1::3])
    got_k, got_s = run(sub)
    inside = np.zeros(R_, bool)
    inside[sub] = True
    assert np.array_equal(got_k[inside], want_k[inside]) and np.array_equal(got_s[inside], want_s[inside])
    assert np.array_equal(got_k[~inside], k_next[~inside]) and not got_s[~inside].any()


def test_ray_skip_adds_to_the_counters(dev):
    ops = _ops()
    o, d, rn, rf, rs = _skip_rays()
    R_ = o.shape[0]
    occ = _occupancy_pattern('empty')
    k = torch.zeros(R_, dtype=torch.int32, device=dev)
    skipped = torch.full((R_,), 7, dtype=torch.int32, device=dev)
    ops.ray_skip(None, _t(o, dev), _t(d, dev), _t(rn, dev), _t(rf, dev), _t(rs, dev), k, _DT, 32, RR.BOX[0], RR.BOX[1], _CELLS, _B,
                 _t(occ, dev), skipped)
    assert np.array_equal(skipped.cpu().numpy(), 7 + (rs + 31) // 32)


# ---- 4. ground truth: the skipped image IS the unskipped image ---------------------------------------------------------------

def _scene(dev_):
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    Rn = _render()
    ds = IndexDataset(SR.SCENE_RES, build_index_table=False)
    vol = _t(SR.scene_volume(), dev_)
    o, d = SR.scene_rays(dev_)
    return Rn, ds, vol, o, d, Rn.TransferFunction(SR.scene_table())


def test_ground_truth_render_with_skipping_is_bit_identical(dev):
    Rn, ds, vol, o, d, tf = _scene(dev)
    assert [float(s) for s in ds.scales] == [float(s) for s in SR.scene_scales()]
    ranges = Rn.BrickRanges.from_volume(ds, vol, brick=SR.SCENE_BRICK)
    want_mm = SR.brick_minmax(SR.scene_volume(), SR.SCENE_BRICK)
    assert np.array_equal(ranges.minmax.cpu().numpy(), want_mm)
    occ = ranges.occupancy(tf)
    assert np.array_equal(occ.cpu().numpy(), SR.occupancy(want_mm, SR.scene_table(), -1.0, 1.0, 1e-5))
    assert ranges.occupancy(tf) is occ and ranges.occupancy(tf, 1e-5) is occ            # cached per (tf, margin)
    for S in (32, 64):
        plain_stats, stats = {}, {}
        plain = Rn.render_from_volume(ds, vol, o, d, tf, step=SR.SCENE_STEP, block_steps=S, stats=plain_stats)
        skipped = Rn.render_from_volume(ds, vol, o, d, tf, step=SR.SCENE_STEP, block_steps=S, stats=stats, skip=ranges)
        assert torch.equal(skipped, plain)
        assert float(plain[:, 3].max()) > 0.3                                           # an image, not a blank
        assert 'skipped_blocks' not in plain_stats
        blocks = plain_stats['samples'] // S
        print('S = %d: %d blocks, %d skipped, samples %d -> %d' % (S, blocks, stats['skipped_blocks'], plain_stats['samples'],
                                                                  stats['samples']))
        assert stats['skipped_blocks'] >= blocks / 4
        # (a ray that turns opaque still jumps, and counts, empty blocks the plain march never reaches: >=)
        assert plain_stats['samples'] > stats['samples'] >= plain_stats['samples'] - S * stats['skipped_blocks']
        chunked = Rn.render_from_volume(ds, vol, o, d, tf, step=SR.SCENE_STEP, block_steps=S, skip=ranges,
                                        max_samples_per_launch=64 * S)
        assert torch.equal(chunked, plain)
        stats = {}
        full = Rn.render_from_volume(ds, vol, o, d, tf, step=SR.SCENE_STEP, block_steps=S, skip=ranges, skip_margin=4.0, stats=stats)
        assert bool(ranges.occupancy(tf, 4.0).all()) and stats['skipped_blocks'] == 0
        assert stats['samples'] == plain_stats['samples'] and stats['live'] == plain_stats['live']
        assert torch.equal(full, plain)
    clear = Rn.TransferFunction(np.concatenate([SR.scene_table()[:, :3], np.zeros((5, 1), F)], 1))
    stats = {}
    img = Rn.render_from_volume(ds, vol, o, d, clear, step=SR.SCENE_STEP, skip=ranges, stats=stats)
    assert torch.equal(img, torch.zeros_like(img)) and stats['samples'] == 0 and stats['live'] == []
    assert stats['skipped_blocks'] > 0


def test_ranges_of_another_box_are_refused(dev):
    Rn, ds, vol, o, d, tf = _scene(dev)
    ranges = Rn.BrickRanges.from_volume(ds, vol, brick=SR.SCENE_BRICK)
    with pytest.raises(ValueError):
        Rn.render(lambda pos: torch.zeros(pos.shape[0], device=dev), o, d, tf, 0.05, [-1.0] * 3, [1.0] * 3, skip=ranges)


# ---- 5. the network: skipping by definition ----------------------------------------------------------------------------------

@pytest.mark.parametrize('shaded', [False, True])
@pytest.mark.parametrize('precision', ['f16x2', 'fp32'])
def test_net_render_with_skipping_is_the_render_told_which_blocks_are_empty(dev, precision, shaded):
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    from latent_feature_grid_compression_amd.visualization.OutputToVTK import field_from_net_fused
    Rn = _render()
    m, _ = build_synth(5, 8, 20, 2, seed=9300, dev=dev)
    m.eval()
    m.precision = precision
    ds = IndexDataset((24, 20, 17), build_index_table=False)
    scales = ds.scales.tolist()
    S = 32
    ranges = Rn.BrickRanges.from_net(ds, m, brick=2, max_slab_voxels=5 * 20 * 17)       # five slabs
    field = field_from_net_fused(ds, m)
    assert np.array_equal(ranges.minmax.cpu().numpy(), SR.brick_minmax(field.cpu().numpy(), 2))
    # transparent on the lower three quarters of the values the network takes, opaque towards the top
    lo, hi = float(field.min()), float(field.max())
    c = np.linspace(0.2, 1.0, 5)
    tf = Rn.TransferFunction(np.stack([c, 0.5 * c, 1.0 - 0.5 * c, np.array([0.0, 0.0, 0.0, 0.0, 40.0])], 1), v_min=lo, v_max=hi)
    margin = 1e-3
    occ = ranges.occupancy(tf, margin)
    assert 0 < int(occ.sum()) < occ.numel()
    o, d = Rn.pinhole_rays((2.3, 1.4, 1.7), (0.1, -0.05, 0.0), (0.0, 0.0, 1.0), 38.0, 24, 20, device=dev)
    shading = 'headlight' if shaded else None
    stats = {}
    got = Rn.render_from_net(ds, m, o, d, tf, shading=shading, skip=ranges, skip_margin=margin, stats=stats)

    net_fn = Rn._net_value_fn(m, values=not shaded)
    seen = [0, 0]

    def told(pos):
        out = net_fn(pos, gradient=shaded)
        values, grad = out if shaded else (out, None)
        occupied = occ.view(-1).bool()[ranges.touched_bricks(pos)].any(1).view(-1, S).any(1)      # per block of S rows
        seen[0] += occupied.numel()
        seen[1] += int((~occupied).sum())
        values = torch.where(occupied.repeat_interleave(S), values.view(-1), torch.full_like(values.view(-1), lo))
        return (values, grad) if shaded else values
    ref_stats = {}
    want = Rn.render(told, o, d, tf, 1.0 / float(ds.max_dim), [-s for s in scales], scales, shading=shading, stats=ref_stats)
    assert torch.equal(got, want)
    # every block the reference evaluates although it is empty is one the skipping render jumps (it also jumps, and
    # counts, empty blocks behind the point where a ray turns opaque, which the reference never reaches)
    assert stats['skipped_blocks'] >= seen[1] > 0
    assert stats['samples'] == ref_stats['samples'] - S * seen[1] and stats['samples'] > 0
    # what the heuristic costs in this image: recorded, not asserted (it measures the ranges, not the kernels)
    plain = Rn.render_from_net(ds, m, o, d, tf, shading=shading)
    print('net %s shaded %d: %d of %d blocks skipped, %d of %d bricks occupied; against the unskipped image: max abs %.3e, '
          'PSNR %.1f dB' % (precision, shaded, seen[1], seen[0], int(occ.sum()), occ.numel(), float((got - plain).abs().max()),
                            Rn.image_psnr(got, plain)))
    assert float(plain[:, 3].max()) > 0.05


# ---- 6. staleness and excess ---------------------------------------------------------------------------------------------------

def test_stale_ranges_are_refused(dev):
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    Rn = _render()
    m, _ = build_synth(5, 8, 20, 2, seed=9301, dev=dev)
    m.eval()
    ds = IndexDataset((24, 20, 17), build_index_table=False)
    ranges = Rn.BrickRanges.from_net(ds, m, brick=4)
    tf = Rn.TransferFunction(SR.scene_table())
    o, d = Rn.pinhole_rays((2.3, 1.4, 1.7), (0.1, -0.05, 0.0), (0.0, 0.0, 1.0), 38.0, 6, 5, device=dev)
    Rn.render_from_net(ds, m, o, d, tf, skip=ranges)
    with torch.no_grad():
        m.final_layer.bias.add_(0.25)
    with pytest.raises(ValueError, match='stale'):
        Rn.render_from_net(ds, m, o, d, tf, skip=ranges)
    Rn.render_from_net(ds, m, o, d, tf, skip=Rn.BrickRanges.from_net(ds, m, brick=4))


def test_supersampled_ranges_are_the_ranges_of_the_finer_lattice(dev):
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    from latent_feature_grid_compression_amd.visualization.OutputToVTK import field_from_net_fused
    Rn = _render()
    m, _ = build_synth(5, 8, 20, 2, seed=9302, dev=dev)
    m.eval()
    m.precision = 'fp32'
    ds = IndexDataset((13, 11, 9), build_index_table=False)
    coarse = Rn.BrickRanges.from_net(ds, m, brick=4)
    fine = Rn.BrickRanges.from_net(ds, m, brick=4, supersample=3)
    assert fine.cells == (36, 30, 24) and fine.brick == 12 and fine.minmax.shape == coarse.minmax.shape
    fine_ds = IndexDataset((37, 31, 25), build_index_table=False)
    assert fine_ds.scales.tolist() == ds.scales.tolist()
    assert np.array_equal(fine.minmax.cpu().numpy(), SR.brick_minmax(field_from_net_fused(fine_ds, m).cpu().numpy(), 12))
    # the finer lattice holds the coarse one up to the rounding of the lattice positions: its ranges are no narrower, within
    # twice the fp32 forward's bound (1e-5 max|v|, |v| <= 1) and the few 1e-7 the positions differ by
    assert bool((fine.minmax[..., 0] <= coarse.minmax[..., 0] + 3e-5).all())
    assert bool((fine.minmax[..., 1] >= coarse.minmax[..., 1] - 3e-5).all())


def test_range_excess_of_the_trilinear_ground_truth_is_within_the_margin(dev):
    Rn, ds, vol, o, d, tf = _scene(dev)
    ranges = Rn.BrickRanges.from_volume(ds, vol, brick=SR.SCENE_BRICK)
    excess = Rn.brick_range_excess(ranges, Rn.volume_value_fn(ds, vol), n=1 << 16, seed=3)
    print('excess of the trilinear sampler over the brick ranges: %.3e' % excess)
    assert 0.0 <= excess <= ranges.default_margin == 1e-5
    # ranges of another field are exceeded by about what the fields differ by
    other = Rn.BrickRanges.from_volume(ds, vol - 0.5, brick=SR.SCENE_BRICK)
    assert 0.3 < Rn.brick_range_excess(other, Rn.volume_value_fn(ds, vol), n=1 << 12) <= 0.5 + 1e-5
    # the torch form of the brick lookup is the restatement's
    pos = (torch.rand((4096, 3), device=dev) * 2.2 - 1.1) * ds.scales.to(dev)
    scales = [float(s) for s in ds.scales]
    want = SR.touched(pos.cpu().numpy(), [-s for s in scales], scales, ranges.cells, ranges.brick)
    assert np.array_equal(ranges.touched_bricks(pos).cpu().numpy(), want)
