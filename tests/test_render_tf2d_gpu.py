"""GPU tests of the 2-D transfer functions over value and gradient magnitude: lfgc_ray_composite2d_f32 against the float64
restatement (tests/tf2d_ref.py) and, for tables that do not depend on the gradient, bit for bit against the 1-D kernel;
the marching loop with a 2-D table against the oracle; empty-space skipping through the value projection; and the joint
histogram against its float32 restatement, exactly.

The compositing bound is 2 x render_ref.composite_bound: the 2-D lookup has two table coordinates and three lerps where
the 1-D one has one of each."""
import numpy as np
import pytest
import torch

import render_ref as RR
import tf2d_ref as T2
from test_hip_forward import build_synth, dev  # noqa: F401
from test_gradient_gpu import _oracle

pytestmark = pytest.mark.gpu
F = np.float32


def _ops():
    from latent_feature_grid_compression_amd import ops
    return ops


def _render():
    from latent_feature_grid_compression_amd.visualization import Render
    return Render


def _t(a, dev_):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev_)


# ---- 1. composite against float64 on the same inputs ----------------------------------------------------------------------

def _run_case(case, dev_, table, shaded, two_d=True, with_grad=True, extra=10, S=None, blocks=None):
    """Chained composite calls on the case's 100 rays (+ `extra` rays that are in no list): ops.ray_composite2d under
    `table` (Kv, Kg, 4), or ops.ray_composite under `table` (K, 4)."""
    ops = _ops()
    S = case['S'] if S is None else S
    nb = case['blocks'] if blocks is None else blocks
    pad = lambda a: np.concatenate([a, a[:extra]])        # noqa: E731
    dirs, tn, tf, n = (_t(pad(case[k]), dev_) for k in ('dirs', 't_near', 't_far', 'n_steps'))
    R_ = 100 + extra
    state = torch.zeros((R_, 4), device=dev_)
    state[:, 3] = 1.0
    state[100:] = torch.tensor([0.1, 0.2, 0.3, 0.4], device=dev_)
    k_next = torch.zeros(R_, dtype=torch.int32, device=dev_)
    k_next[100:] = 7
    live = torch.arange(100, dtype=torch.int32, device=dev_)
    table = _t(table, dev_)
    for b in range(nb):
        v = _t(case['values'][:, b * S:(b + 1) * S].reshape(-1), dev_)
        g = _t(case['grads'][:, b * S:(b + 1) * S].reshape(-1, 3), dev_) if with_grad else None
        if two_d:
            ops.ray_composite2d(live, v, g, dirs, tn, tf, n, k_next, RR.DT, S, table, -1.0, 1.0, T2.G_MAX, case['limit'], state,
                                shade=shaded)
        else:
            ops.ray_composite(live, v, g, dirs, tn, tf, n, k_next, RR.DT, S, table, -1.0, 1.0, case['limit'], state)
    return state, k_next


@pytest.mark.parametrize('shaded', [False, True])
@pytest.mark.parametrize('limit', [0.95, 1.0])
def test_composite2d_matches_float64(dev, limit, shaded):
    case = T2.composite_case2d(limit, shaded)
    state, k_next = _run_case(case, dev, case['table'], shaded)
    state, k_next = state.cpu().numpy(), k_next.cpu().numpy()
    out = RR.left_out(case['margin'], 1e-5)
    assert out.sum() <= 0.02 * out.size
    steps = np.minimum(case['n_steps'], case['blocks'] * case['S'])
    bound = RR.composite_bound(steps)[:, None]
    err = np.abs(state[:100].astype(np.float64) - case['ref'])
    worst = (err / bound)[~out].max()
    print('composite2d limit %g shaded %d: max err %.3e, max err / composite_bound %.3f (allowed: 2), %d rays left out'
          % (limit, shaded, err[~out].max(), worst, out.sum()))
    assert worst <= 2.0
    assert np.array_equal(k_next[:100], np.full(100, case['blocks'] * case['S'], np.int32))
    # rays in no list are untouched
    assert np.array_equal(k_next[100:], np.full(10, 7, np.int32))
    assert np.array_equal(state[100:], np.tile(np.array([0.1, 0.2, 0.3, 0.4], F), (10, 1)))
    # T never increases and stays a transmittance
    assert (state[:100, 3] <= 1.0).all() and (state[:100, 3] >= 0.0).all()


def test_transmittance_never_increases_from_call_to_call(dev):
    case = T2.composite_case2d(0.95, True)
    before = np.ones(100, F)
    for nb in (1, 2, 3):
        state, _ = _run_case(case, dev, case['table'], True, blocks=nb)
        T = state[:100, 3].cpu().numpy()
        assert (T <= before).all() and (T >= 0.0).all()
        before = T


# ---- 2. a table that does not depend on g: the bits of the 1-D kernel ---------------------------------------------------------

@pytest.mark.parametrize('shaded', [False, True])
@pytest.mark.parametrize('Kg', [5, 2])
def test_a_table_constant_along_g_gives_the_bits_of_the_1d_kernel(dev, Kg, shaded):
    case = RR.composite_case(0.95, True)
    table2 = np.ascontiguousarray(np.repeat(case['table'][:, None, :], Kg, 1))
    got, k2 = _run_case(case, dev, table2, shaded)
    want, k1 = _run_case(case, dev, case['table'], shaded, two_d=False, with_grad=shaded)      # grad=None when unshaded
    assert torch.equal(got, want) and torch.equal(k2, k1)
    assert float((1.0 - want[:100, 3]).max()) >= 0.95                 # the contribution rule was exercised


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shaded', [False, True])
def test_single_step_rays_at_the_clamps_of_both_axes(dev, shaded):
    """v in {below v_min, v_min, v_max, above} x |g| in {0, g_max, above g_max}: 12 rays of one step each."""
    ops = _ops()
    rng = np.random.default_rng(31)
    table = np.concatenate([rng.uniform(0, 1, (7, 5, 3)), rng.uniform(0, 6, (7, 5, 1))], 2).astype(F)
    v_min, v_max, g_max = -0.5, 0.75, 1.5
    vs = np.array([-0.9, v_min, v_max, 2.0], F)
    gs = np.array([[0.0, 0.0, 0.0], [0.0, g_max, 0.0], [1.0, -2.0, 2.0]], F)
    v = np.repeat(vs, 3)
    g = np.tile(gs, (4, 1))
    R_, S = 12, 32
    dirs = rng.normal(size=(R_, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F)
    tn = rng.uniform(0.5, 1.5, R_).astype(F)
    tf = (tn + F(0.8) * F(RR.DT)).astype(F)                           # one short segment
    n = np.ones(R_, np.int32)
    values = np.zeros((R_, S), F)
    grads = np.zeros((R_, S, 3), F)
    values[:, 0], grads[:, 0] = v, g
    values[:, 1:], grads[:, 1:] = 0.3, 0.7                             # padding rows: never used
    state = torch.zeros((R_, 4), device=dev)
    state[:, 3] = 1.0
    k_next = torch.zeros(R_, dtype=torch.int32, device=dev)
    ops.ray_composite2d(torch.arange(R_, dtype=torch.int32, device=dev), _t(values.reshape(-1), dev), _t(grads.reshape(-1, 3), dev),
                        _t(dirs, dev), _t(tn, dev), _t(tf, dev), _t(n, dev), k_next, RR.DT, S, _t(table, dev), v_min, v_max, g_max,
                        1.0, state, shade=shaded)
    ref, _ = T2.composite2d(values, grads, dirs, tn, tf, n, RR.DT, table, v_min, v_max, g_max, 1.0, shaded)
    err = np.abs(state.cpu().numpy().astype(np.float64) - ref)
    print('single-step rays shaded %d: max err / composite_bound %.3f (allowed: 2)' % (shaded, err.max() / RR.composite_bound(1)))
    assert err.max() <= 2.0 * RR.composite_bound(1)
    # and the corners are what they should be: the clamped samples see the end rows alone
    length = np.float64(tf) - np.float64(tn)
    corner = {(0, 0): table[0, 0], (0, 2): table[0, 4], (3, 0): table[6, 0], (3, 2): table[6, 4], (1, 1): table[0, 4],
              (2, 1): table[6, 4]}
    for (a, b), rgba in corner.items():
        r = 3 * a + b
        assert abs((1.0 - ref[r, 3]) - (1.0 - np.exp(-np.float64(rgba[3]) * length[r]))) <= 1e-12
    assert np.array_equal(k_next.cpu().numpy(), np.full(R_, S, np.int32))


def test_one_block_of_64_against_two_of_32(dev):
    case = T2.composite_case2d(1.0, True)
    a, ka_ = _run_case(case, dev, case['table'], True, S=64, blocks=1)
    b, kb_ = _run_case(case, dev, case['table'], True, S=32, blocks=2)
    assert torch.equal(ka_, kb_)
    bound = RR.composite_bound(np.minimum(case['n_steps'], 64))[:, None]
    diff = np.abs(a[:100].cpu().numpy().astype(np.float64) - b[:100].cpu().numpy().astype(np.float64))
    print('S = 64 against 2 x S = 32: max difference / composite_bound %.3f (allowed: 1)' % (diff / bound).max())
    assert (diff / bound).max() <= 1.0


# ---- 4. end to end against the oracle -------------------------------------------------------------------------------------

_E2E_G_MAX = 0.64      # the 75th percentile of the oracle's |gradient| over this view's samples: a quarter clamps above it


def _e2e_table():
    """Seed 101: the float64 reference alone leaves 1 of 304 rays within 1e-4 of the limit, and rays do reach the limit."""
    rng = np.random.default_rng(101)
    return np.concatenate([rng.uniform(0, 1, (7, 5, 3)), rng.uniform(0, 6, (7, 5, 1))], 2).astype(F)


def _view(dev_):
    o, d = _render().pinhole_rays((2.3, 1.4, 1.7), (0.1, -0.05, 0.0), (0.0, 0.0, 1.0), 38.0, 24, 20, device=dev_)
    return o, d, d / d.norm(dim=1, keepdim=True)


def _all_blocks(o, dn, box, step, S=32):
    """Clip + the positions of EVERY block of every hit ray from the device."""
    ops, Rn = _ops(), _render()
    tn, tf, n = ops.ray_clip(o, dn, box[0], box[1], step, Rn.max_steps_for(box[0], box[1], step))
    hit = torch.nonzero(n > 0).view(-1).to(torch.int32)
    k_next = torch.zeros_like(n)
    blocks = []
    for b in range((int(n.max()) + S - 1) // S):
        blocks.append(ops.ray_samples(hit, o, dn, tn, tf, n, k_next, step, S).view(hit.numel(), S, 3))
        k_next += S
    h = hit.long()
    return hit, tn[h].cpu().numpy(), tf[h].cpu().numpy(), n[h].cpu().numpy(), torch.cat(blocks, 1)


_E2E = {}


def _e2e(dev_):
    """The model, the view and the oracle's values and gradients at the device's own positions, once for both cases."""
    if not _E2E:
        from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
        m, _ = build_synth(5, 8, 20, 2, seed=9100 + 5 + 20, dev=dev_)
        m.eval()
        ds = IndexDataset((33, 25, 17), build_index_table=False)          # scales (1, 0.75, 0.5), default step 1/32
        scales = ds.scales.tolist()
        box = ([-s for s in scales], scales)
        step = 1.0 / float(ds.max_dim)
        o, d, dn = _view(dev_)
        hit, tn, tf_, n, pos = _all_blocks(o, dn, box, step)
        n_hit, M = pos.shape[:2]
        y, g = _oracle(m)(pos.reshape(-1, 3))
        _E2E.update(m=m, ds=ds, step=step, o=o, d=d, hit=hit.cpu().numpy(), tn=tn, tf=tf_, n=n,
                    dirs=dn[hit.long()].cpu().numpy(), v=np.clip(y.astype(np.float64), -1.0, 1.0).reshape(n_hit, M),
                    g=g.astype(np.float64).reshape(n_hit, M, 3))
    return _E2E


@pytest.mark.parametrize('shaded', [False, True])
def test_render_from_net_with_a_2d_table_matches_the_oracle(dev, shaded):
    Rn = _render()
    e = _e2e(dev)
    limit, ka, kd = 0.99, 0.3, 0.7
    table = _e2e_table()
    tf = Rn.TransferFunction2D(table, g_max=_E2E_G_MAX)
    got = Rn.render_from_net(e['ds'], e['m'], e['o'], e['d'], tf, opacity_limit=limit,
                             shading='headlight' if shaded else None).cpu().numpy()
    v, g, hit, n = e['v'], e['g'], e['hit'], e['n']
    gn = np.sqrt((g * g).sum(2))
    assert 0.05 < (gn > _E2E_G_MAX).mean() < 0.6                      # both sides of the g clamp are seen
    args = (e['dirs'], e['tn'], e['tf'], n, e['step'], table, -1.0, 1.0, _E2E_G_MAX, limit, shaded, ka, kd)
    ref, margin = T2.composite2d(v, g, *args)
    # what the project's own forward bound (1e-5 max|v|; 2e-5 max|g| for gradients) is worth in this image
    rng = np.random.default_rng(5)
    v2 = v + 1e-5 * np.abs(v).max() * rng.choice([-1.0, 1.0], v.shape)
    g2 = g + 2e-5 * np.abs(g).max() * rng.choice([-1.0, 1.0], g.shape)
    ref2, _ = T2.composite2d(v2, g2, *args)
    delta = np.abs(ref2 - ref).max()
    out = RR.left_out(margin, 1e-4)
    assert out.sum() <= 0.02 * out.size
    R_ = e['o'].shape[0]
    want = np.zeros((R_, 4))
    want[hit] = ref
    want[hit, 3] = 1.0 - ref[:, 3]
    err = np.abs(got.astype(np.float64) - want)
    bound = np.full((R_, 1), 4.0 * delta)
    bound[hit, 0] += 2.0 * RR.composite_bound(n)
    keep = np.ones(R_, bool)
    keep[hit[out]] = False
    print('render 2-D shaded %d: delta %.3e, max err %.3e, max err / bound %.3f, %d of %d rays left out, %d hit, max opacity %.4f'
          % (shaded, delta, err[keep].max(), (err / bound)[keep].max(), out.sum(), out.size, len(hit), want[:, 3].max()))
    assert len(hit) > 100 and int(n.max()) > 64
    assert (err / bound)[keep].max() <= 1.0
    assert np.array_equal(got[np.setdiff1d(np.arange(R_), hit)], np.zeros((R_ - len(hit), 4), F))


def test_a_value_fn_without_gradients_is_refused(dev):
    Rn = _render()
    o, d, _ = _view(dev)
    tf = Rn.TransferFunction2D(_e2e_table(), g_max=1.0)
    box = ([-1.0, -0.75, -0.5], [1.0, 0.75, 0.5])
    for shading in (None, 'headlight'):
        with pytest.raises(ValueError, match='2-D transfer function needs value_fn to return \\(values, gradients\\)'):
            Rn.render(lambda pos: torch.zeros(pos.shape[0], device=dev), o, d, tf, 0.05, *box, shading=shading)
        with pytest.raises(ValueError, match='2-D transfer function needs'):
            Rn.render(lambda pos: (torch.zeros(pos.shape[0], device=dev), None), o, d, tf, 0.05, *box, shading=shading)
    m, _ = build_synth(5, 8, 20, 2, seed=9125, dev=dev)
    m.train()
    with pytest.raises(ValueError, match='eval'):
        Rn.render_from_net([1.0, 0.75, 0.5], m, o, d, tf, step=0.05)


# ---- 5. empty-space skipping through the value projection ------------------------------------------------------------------

def _half_empty_volume():
    """(33, 25, 17): -0.8 in the lower x half, smooth and positive elsewhere."""
    x, y, z = np.meshgrid(np.arange(33) / 32.0, np.arange(25) / 24.0, np.arange(17) / 16.0, indexing='ij')
    smooth = 0.5 + 0.25 * np.sin(5.0 * x + 1.0) * np.cos(4.0 * y) + 0.15 * np.sin(6.0 * z + 2.0 * x)       # in [0.1, 0.9]
    return np.where(x < 0.5, -0.8, smooth).astype(F)


def test_skipping_under_a_2d_table_is_bit_identical(dev):
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    Rn = _render()
    vol_np = _half_empty_volume()
    assert vol_np[16:].min() > 0.0 and vol_np[16:].max() < 1.0
    ds = IndexDataset((33, 25, 17), build_index_table=False)
    vol = _t(vol_np, dev)
    o, d, _ = _view(dev)
    ranges = Rn.BrickRanges.from_volume(ds, vol, brick=4)
    rng = np.random.default_rng(12)
    table = np.concatenate([rng.uniform(0, 1, (9, 4, 3)), rng.uniform(1, 6, (9, 4, 1))], 2).astype(F)
    # (a) no extinction in any entry of the value rows below 0 (rows 0..3 of 9 over [-1, 1])
    a = table.copy()
    a[:4, :, 3] = 0.0
    tf_a = Rn.TransferFunction2D(a, g_max=8.0)
    plain_stats, stats = {}, {}
    plain = Rn.render_from_volume(ds, vol, o, d, tf_a, stats=plain_stats)
    skipped = Rn.render_from_volume(ds, vol, o, d, tf_a, stats=stats, skip=ranges)
    assert torch.equal(skipped, plain)
    assert float(plain[:, 3].max()) > 0.3                             # an image, not a blank
    print('2-D skip: %d blocks skipped, samples %d -> %d' % (stats['skipped_blocks'], plain_stats['samples'], stats['samples']))
    assert stats['skipped_blocks'] > 0 and stats['samples'] < plain_stats['samples']
    occ = ranges.occupancy(tf_a)
    assert 0 < int(occ.sum()) < occ.numel() and ranges.occupancy(tf_a) is occ
    assert torch.equal(occ, ranges.occupancy(tf_a.value_projection()))
    # (b) transparent in the lowest g row alone: the bricks bound the value only, nothing can be skipped
    b = table.copy()
    b[:, 0, 3] = 0.0
    tf_b = Rn.TransferFunction2D(b, g_max=8.0)
    plain_stats, stats = {}, {}
    plain = Rn.render_from_volume(ds, vol, o, d, tf_b, stats=plain_stats)
    skipped = Rn.render_from_volume(ds, vol, o, d, tf_b, stats=stats, skip=ranges)
    assert stats['skipped_blocks'] == 0 and stats['samples'] == plain_stats['samples']
    assert torch.equal(skipped, plain)
    assert float(plain[:, 3].max()) > 0.3
    with pytest.raises(ValueError, match='shading'):
        Rn.render_from_volume(ds, vol, o, d, tf_a, shading='headlight')


# ---- 6. the joint histogram ---------------------------------------------------------------------------------------------------

_HIST_N = 50037


def _hist_samples():
    rng = np.random.default_rng(606)
    v = rng.normal(0.0, 0.7, _HIST_N).astype(F)                       # ~ 15 % outside [-1, 1]
    g = rng.normal(0.0, 0.8, (_HIST_N, 3)).astype(F)                  # |g| above g_max = 2 for ~ 10 %
    g[rng.uniform(size=_HIST_N) < 0.1] = 0.0
    v[:3] = [-1.0, 1.0, 0.0]                                         # on the ends of the range and on an edge
    return v, g


@pytest.mark.parametrize('bins', [(8, 5), (64, 64)])
def test_joint_histogram_equals_the_restatement(dev, bins):
    ops = _ops()
    v, g = _hist_samples()
    assert (np.abs(v) > 1).mean() > 0.05 and (T2.grad_norm_f32(g) > 2.0).mean() > 0.02 and (T2.grad_norm_f32(g) == 0).mean() > 0.05
    want = T2.histogram(v, g, bins, -1.0, 1.0, 2.0)
    vd, gd = _t(v, dev), _t(g, dev)
    counts = ops.joint_histogram(vd, gd, bins, -1.0, 1.0, 2.0)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == bins
    got = counts.cpu().numpy()
    print('joint histogram %s: L1 difference to the restatement %d of %d samples' % (bins, np.abs(got - want).sum(), _HIST_N))
    assert got.sum() == _HIST_N
    assert np.array_equal(got, want)
    # a second call accumulates
    again = ops.joint_histogram(vd, gd, bins, -1.0, 1.0, 2.0, counts)
    assert again is counts and np.array_equal(counts.cpu().numpy(), 2 * want)
    # two unequal parts are the whole
    parts = ops.joint_histogram(vd[:12345], gd[:12345], bins, -1.0, 1.0, 2.0)
    ops.joint_histogram(vd[12345:], gd[12345:], bins, -1.0, 1.0, 2.0, parts)
    assert np.array_equal(parts.cpu().numpy(), want)


def test_joint_histogram_checks_its_arguments(dev):
    ops = _ops()
    v, g = torch.zeros(10, device=dev), torch.zeros(10, 3, device=dev)
    for bad in ((0, 4), (129, 128)):
        with pytest.raises(ValueError):
            ops.joint_histogram(v, g, bad, -1.0, 1.0, 2.0)
    with pytest.raises(ValueError):
        ops.joint_histogram(v, g, (4, 4), 1.0, 1.0, 2.0)
    with pytest.raises(ValueError):
        ops.joint_histogram(v, g, (4, 4), -1.0, 1.0, 0.0)
    with pytest.raises(ValueError):
        ops.joint_histogram(v, g[:5], (4, 4), -1.0, 1.0, 2.0)
    with pytest.raises(ValueError):
        ops.joint_histogram(v, g, (4, 4), -1.0, 1.0, 2.0, torch.zeros(4, 4, device=dev))      # not int64
    empty = ops.joint_histogram(v[:0], g[:0], (4, 4), -1.0, 1.0, 2.0)
    assert int(empty.sum()) == 0
    assert int(ops.joint_histogram(v, g, (128, 128), -1.0, 1.0, 2.0)[64, 0]) == 10      # the largest table: 64 KB of LDS


def test_joint_histogram_from_net_and_from_volume(dev):
    from latent_feature_grid_compression_amd.visualization.OutputToVTK import _row_chunks, gradient_ground_truth
    ops, Rn = _ops(), _render()
    e = _e2e(dev)
    m, ds = e['m'], e['ds']
    res = ds.vol_res_touple
    pos = ops.lattice_slab_positions(res, 0, res[0], 32, ds.scales.tolist(), dev)
    v, g = m.value_and_gradient(pos)
    top = float(g.norm(dim=1).max())
    counts, g_max = Rn.joint_histogram_from_net(ds, m, bins=(8, 5))
    assert g_max == top and int(counts.sum()) == res[0] * res[1] * res[2]
    assert torch.equal(counts, ops.joint_histogram(v.view(-1), g, (8, 5), -1.0, 1.0, top))
    assert int((counts > 0).sum()) > 5
    # a range that clamps on both axes, and a stash limit that forces several chunks: the same bits
    small = 1 << 16
    assert len(_row_chunks(m, res[0], res[1] * res[2], small)) > 3
    want = ops.joint_histogram(v.view(-1), g, (64, 64), -0.1, 0.05, 0.5)
    for stash in (1 << 30, small):
        got, gm = Rn.joint_histogram_from_net(ds, m, bins=(64, 64), v_range=(-0.1, 0.05), g_max=0.5, max_stash_bytes=stash)
        assert gm == 0.5 and torch.equal(got, want)
    m.train()
    with pytest.raises(ValueError, match='eval'):
        Rn.joint_histogram_from_net(ds, m)
    m.eval()
    # the ground truth: the volume's own values and the central differences of gradient_ground_truth
    vol = _t(_half_empty_volume(), dev)
    gg = gradient_ground_truth(ds, vol)
    for slab in (1 << 22, 3 * res[1] * res[2]):
        got, gm = Rn.joint_histogram_from_volume(ds, vol, bins=(8, 5), max_slab_voxels=slab)
        assert gm == float(gg.norm(dim=1).max())
        assert torch.equal(got, ops.joint_histogram(vol.view(-1), gg, (8, 5), -1.0, 1.0, gm))
    assert int(got.sum()) == vol.numel() and int(got[0].sum()) >= 16 * 25 * 17          # the empty half sits in the lowest value bin
