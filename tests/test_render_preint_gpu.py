"""GPU tests of pre-integrated classification: lfgc_ray_composite_preint_f32 against the float64 restatement
(tests/preint_ref.py) over chained calls, jumps of k_next between calls, one call of 64 against two of 32, the edges of the
table, the linear ramp the midpoint rule misses, the marching loop against the oracle, and empty-space skipping.

The compositing bound is k x render_ref.composite_bound with k = 2 max(1, ratio), ratio = what the float32 restatement of
the contract alone differs from the float64 one on the same inputs (preint_ref.tolerance_factor): the slab mean has two
table coordinates, up to two brackets and two divisions where the midpoint lookup has one coordinate and one lerp.  k is
computed from the restatement, never from the kernel."""
import numpy as np
import pytest
import torch

import preint_ref as P
import render_ref as RR
from test_hip_forward import build_synth, dev  # noqa: F401
from test_render_tf2d_gpu import _e2e, _half_empty_volume, _view

pytestmark = pytest.mark.gpu
F = np.float32
EXTRA = 10                                                             # rays that are in no list
EXTRA_STATE, EXTRA_K, EXTRA_CARRY = (0.1, 0.2, 0.3, 0.4), 7, (0.5, 3)


def _ops():
    from latent_feature_grid_compression_amd import ops
    return ops


def _render():
    from latent_feature_grid_compression_amd.visualization import Render
    return Render


def _t(a, dev_):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev_)


def _rows(a, k_next, S):
    """a (R, M, ...) -> (R, S, ...): columns k_next[r] .. k_next[r] + S - 1 of every ray, zeros past M (padding rows)."""
    R, M = a.shape[:2]
    k = k_next[:, None].astype(np.int64) + np.arange(S)[None, :]
    out = a[np.arange(R)[:, None], np.minimum(k, M - 1)]
    out[k >= M] = 0
    return out


def _run(case, dev_, shaded, S=None, blocks=None, jumps=False, dt=RR.DT, composite=None):
    """Chained ops.ray_composite_preint calls on the case's rays (+ EXTRA rays that are in no list).  ``jumps``: k_next is
    moved on the host as P.preint_case(jumps=True) describes.  Returns numpy (state, k_next, carry_v, carry_k) and T after
    every call."""
    ops, Rn = _ops(), _render()
    S = case['S'] if S is None else S
    nb = case['blocks'] if blocks is None else blocks
    R = case['values'].shape[0]
    pad = lambda a: np.concatenate([a, a[:EXTRA]])        # noqa: E731
    dirs, tn, tf, n = (_t(pad(case[k]), dev_) for k in ('dirs', 't_near', 't_far', 'n_steps'))
    state = torch.zeros((R + EXTRA, 4), device=dev_)
    state[:, 3] = 1.0
    state[R:] = torch.tensor(EXTRA_STATE, device=dev_)
    k_next = torch.zeros(R + EXTRA, dtype=torch.int32, device=dev_)
    k_next[R:] = EXTRA_K
    carry_v = torch.zeros(R + EXTRA, device=dev_)
    carry_k = torch.full((R + EXTRA,), -1, dtype=torch.int32, device=dev_)
    carry_v[R:], carry_k[R:] = EXTRA_CARRY
    live = torch.arange(R, dtype=torch.int32, device=dev_)
    tf_ = Rn.TransferFunction(case['table'], case['v_min'], case['v_max'])
    table, pre = tf_.on(dev_), tf_.integral_on(dev_)
    T = []
    for b in range(nb):
        if jumps and b < 2:
            k_next[(1 - b):R:P.JUMP_EVERY] += S                       # before the first call: rays 1, 4, ...; then rays 0, 3, ...
        at = k_next[:R].cpu().numpy()
        v = _t(_rows(case['values'], at, S).reshape(-1), dev_)
        g = _t(_rows(case['grads'], at, S).reshape(-1, 3), dev_) if shaded else None
        if composite is not None:
            composite(live, v, g, dirs, tn, tf, n, k_next, dt, S, table, case['v_min'], case['v_max'], case['limit'], state)
        else:
            ops.ray_composite_preint(live, v, g, dirs, tn, tf, n, k_next, dt, S, table, pre, case['v_min'], case['v_max'],
                                     case['limit'], state, carry_v, carry_k)
        T.append(state[:R, 3].cpu().numpy())
    return state.cpu().numpy(), k_next.cpu().numpy(), carry_v.cpu().numpy(), carry_k.cpu().numpy(), T


def _check_against_ref(case, got, what, dt=RR.DT):
    state, k_next, carry_v, carry_k, T = got
    R = case['values'].shape[0]
    k, ratio = P.tolerance_factor(case, dt)
    out = RR.left_out(case['margin'], 1e-5)
    assert out.sum() <= 0.02 * out.size
    bound = RR.composite_bound(case['steps'])[:, None]
    err = np.abs(state[:R].astype(np.float64) - case['ref'])
    worst = (err / bound)[~out].max()
    print('%s: max err %.3e, max err / composite_bound %.3f (allowed: k = %.2f, float32 restatement alone: %.3f), %d rays left out'
          % (what, err[~out].max(), worst, k, ratio, out.sum()))
    assert ratio < 4.0
    assert worst <= k
    # rays in no list keep their state, k_next and carry bit for bit
    assert np.array_equal(state[R:], np.tile(np.array(EXTRA_STATE, F), (EXTRA, 1)))
    assert np.array_equal(k_next[R:], np.full(EXTRA, EXTRA_K, np.int32))
    assert np.array_equal(carry_v[R:], np.full(EXTRA, EXTRA_CARRY[0], F)) and np.array_equal(carry_k[R:], np.full(EXTRA, EXTRA_CARRY[1], np.int32))
    # T is a transmittance and never increases from call to call
    before = np.ones(R, F)
    for t in T:
        assert (t <= before).all() and (t >= 0.0).all()
        before = t


def _expected_carry(case, k_end):
    """(carry_k, carry_v) after the calls: the last row with k < n_steps that was composited."""
    R, M = case['values'].shape
    k = np.arange(M)[None, :]
    done = case['evaluated'] & (k < case['n_steps'][:, None]) & (k < k_end[:, None])
    last = np.where(done.any(1), M - 1 - np.argmax(done[:, ::-1], 1), -1)
    return last.astype(np.int32), np.where(last >= 0, case['values'][np.arange(R), np.maximum(last, 0)], 0).astype(F)


# ---- 1. the kernel against float64 -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('walk', [False, True])
@pytest.mark.parametrize('shaded', [False, True])
@pytest.mark.parametrize('limit', [0.95, 1.0])
def test_composite_preint_matches_float64(dev, limit, shaded, walk):
    case = P.preint_case(limit, shaded, walk)
    got = _run(case, dev, shaded)
    _check_against_ref(case, got, 'preint limit %g shaded %d walk %d' % (limit, shaded, walk))
    R = case['values'].shape[0]
    assert np.array_equal(got[1][:R], np.full(R, case['blocks'] * case['S'], np.int32))
    want_k, want_v = _expected_carry(case, got[1][:R])
    assert np.array_equal(got[3][:R], want_k) and np.array_equal(got[2][:R], want_v)
    if limit < 1.0:
        assert (1.0 - got[0][:R, 3] >= limit).sum() >= 10              # the contribution rule was exercised


# ---- 2. jumps of k_next between calls ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('shaded', [False, True])
@pytest.mark.parametrize('limit', [0.95, 1.0])
def test_jumps_of_k_next_open_a_new_half_slab(dev, limit, shaded):
    case = P.preint_case(limit, shaded, False, True)
    got = _run(case, dev, shaded, jumps=True)
    _check_against_ref(case, got, 'preint with jumps limit %g shaded %d' % (limit, shaded))
    R, S = case['values'].shape[0], case['S']
    want = np.full(R, 3 * S, np.int32)
    want[0::P.JUMP_EVERY] += S
    want[1::P.JUMP_EVERY] += S
    assert np.array_equal(got[1][:R], want)
    want_k, want_v = _expected_carry(case, got[1][:R])
    assert np.array_equal(got[3][:R], want_k) and np.array_equal(got[2][:R], want_v)


# ---- 3. one call of 64 against two of 32 -------------------------------------------------------------------------------------

def test_one_block_of_64_against_two_of_32(dev):
    case = P.preint_case(1.0, True, True)
    a = _run(case, dev, True, S=64, blocks=1)
    b = _run(case, dev, True, S=32, blocks=2)
    R = case['values'].shape[0]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    bound = RR.composite_bound(np.minimum(case['n_steps'], 64))[:, None]
    diff = np.abs(a[0][:R].astype(np.float64) - b[0][:R].astype(np.float64))
    print('S = 64 against 2 x S = 32: max difference / composite_bound %.3f (allowed: 1); bit for bit: %s'
          % ((diff / bound).max(), np.array_equal(a[0], b[0])))
    assert (diff / bound).max() <= 1.0


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------

def _edge_case(K, shaded):
    """Eight short rays: single steps at and beyond both clamps, equal values, the whole table in one slab, NaNs."""
    rng = np.random.default_rng(41)
    table = np.concatenate([rng.uniform(0, 1, (K, 3)), rng.uniform(0.5, 6, (K, 1))], 1).astype(F)
    v_min, v_max = -0.5, 0.75
    n = np.array([1, 1, 1, 1, 3, 2, 3, 4], np.int32)
    R_, S = len(n), 32
    values = np.full((R_, S), 0.3, F)                                  # padding rows: never used
    values[:4, 0] = [-0.9, v_min, v_max, 2.0]
    values[4, :3] = 0.2                                                # a slab whose two values are equal
    values[5, :2] = [-0.9, 2.0]                                        # a slab spanning the whole table
    values[6, :3] = [np.nan, 0.1, np.nan]                              # a NaN lands in row 0
    values[7, :4] = rng.uniform(v_min, v_max, 4)
    dirs = rng.normal(size=(R_, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(F)
    grads = rng.normal(size=(R_, S, 3)).astype(F) if shaded else None
    tn = rng.uniform(0.5, 1.5, R_).astype(F)
    tf = (tn + (n - F(0.2)).astype(F) * F(RR.DT)).astype(F)            # the last segment is short
    case = dict(values=values, grads=grads, dirs=dirs, t_near=tn, t_far=tf, n_steps=n, table=table, v_min=v_min, v_max=v_max,
                limit=1.0, evaluated=None, steps=n, S=S, blocks=1)
    case['ref'], case['margin'] = P.composite_preint(values, grads, dirs, tn, tf, n, RR.DT, table, v_min, v_max, 1.0)
    case['margin'] = np.full(R_, np.inf)                               # limit 1: no ray is decided by rounding
    return case


@pytest.mark.parametrize('shaded', [False, True])
@pytest.mark.parametrize('K', [7, 2])
def test_edges_of_the_table(dev, K, shaded):
    case = _edge_case(K, shaded)
    got = _run(case, dev, shaded)
    assert np.isfinite(case['ref']).all() and np.isfinite(got[0]).all()
    _check_against_ref(dict(case, evaluated=np.ones(case['values'].shape, bool)), got, 'edges K = %d shaded %d' % (K, shaded))
    # the clamped single-step rays see the end rows alone, over the whole chord
    length = np.float64(case['t_far']) - np.float64(case['t_near'])
    for r, row in ((0, 0), (1, 0), (2, K - 1), (3, K - 1)):
        assert abs((1.0 - case['ref'][r, 3]) - (1.0 - np.exp(-np.float64(case['table'][row, 3]) * length[r]))) <= 1e-12
    # the NaN ray is the ray with v_min in the NaNs' place
    swapped = case['values'].copy()
    swapped[6, [0, 2]] = case['v_min']
    ref2, _ = P.composite_preint(swapped, case['grads'], case['dirs'], case['t_near'], case['t_far'], case['n_steps'], RR.DT,
                                 case['table'], case['v_min'], case['v_max'], 1.0)
    assert np.array_equal(ref2[6], case['ref'][6])
    assert np.array_equal(got[1][:8], np.full(8, 32, np.int32)) and np.array_equal(got[3][:8], case['n_steps'] - 1)


# ---- 5. the linear ramp: what the midpoint rule misses -----------------------------------------------------------------------

@pytest.mark.parametrize('step,miss', [(0.16, 0.04), (0.3, 0.5)])
def test_linear_ramp_on_the_device(dev, step, miss):
    c = P.ramp_case(step)
    n = c['n_steps']
    case = dict(values=c['values32'], grads=None, dirs=c['dirs'], t_near=c['t_near'], t_far=c['t_far'], n_steps=n, table=c['table'],
                v_min=-1.0, v_max=1.0, limit=1.0, evaluated=None, steps=n, S=c['M'], blocks=1)
    case['ref'], _ = P.composite_preint(c['values32'], None, c['dirs'], c['t_near'], c['t_far'], n, step, c['table'], -1.0, 1.0, 1.0)
    case['margin'] = np.full(len(n), np.inf)
    got = _run(case, dev, False, dt=step)
    _check_against_ref(dict(case, evaluated=np.ones(case['values'].shape, bool)), got, 'ramp at step %g' % step, dt=step)
    k, _ = P.tolerance_factor(dict(case, evaluated=np.ones(case['values'].shape, bool)), step)
    opacity = 1.0 - got[0][:len(n), 3].astype(np.float64)
    # a float32 value is off the line by its own rounding (2^-24 * 0.9) and by the rounding of its float32 position
    # (slope * half an ulp of 2.7): 1.8e-7; a slab's difference of 0.17 or more is then off by 2.1e-6 of itself, and
    # tau_bar * len summed over the ray is 2.36 -> the restatement on these values is within 1e-5 of the closed form
    closed = np.abs(opacity - c['opacity']).max()
    print('ramp at step %g: device opacity %.7f, exact %.7f, difference %.3e' % (step, opacity[0], c['opacity'], closed))
    assert np.abs((1.0 - case['ref'][:, 3]) - c['opacity']).max() <= 1e-5
    assert closed <= k * RR.composite_bound(n[0]) + 1e-5
    mid = _run(case, dev, False, dt=step, composite=_ops().ray_composite)
    off = np.abs((1.0 - mid[0][:len(n), 3].astype(np.float64)) - c['opacity']).min()
    print('ramp at step %g: the midpoint rule is off by %.3f' % (step, off))
    assert off > miss


# ---- 6. end to end against the oracle ---------------------------------------------------------------------------------------

_E2E_LIMIT = 0.95


def _e2e_table():
    """Seed 101 with extinction <= 12 under the limit 0.95: the float64 reference alone leaves 1 of 304 rays within 1e-4 of
    the limit (a ray near the limit gains T * alpha per sample, so a low limit and a large alpha keep the rays apart), and
    238 rays reach the limit."""
    rng = np.random.default_rng(101)
    return np.concatenate([rng.uniform(0, 1, (7, 3)), rng.uniform(0, 12, (7, 1))], 1).astype(F)


@pytest.mark.parametrize('shaded', [False, True])
def test_render_from_net_preintegrated_matches_the_oracle(dev, shaded):
    Rn = _render()
    e = _e2e(dev)
    limit, ka, kd = _E2E_LIMIT, 0.3, 0.7
    table = _e2e_table()
    tf = Rn.TransferFunction(table)
    kw = dict(opacity_limit=limit, shading='headlight' if shaded else None)
    image = Rn.render_from_net(e['ds'], e['m'], e['o'], e['d'], tf, preintegrated=True, **kw)
    got = image.cpu().numpy()
    v, g, hit, n = e['v'], e['g'] if shaded else None, e['hit'], e['n']
    args = (e['dirs'], e['tn'], e['tf'], n, e['step'], table, -1.0, 1.0, limit, ka, kd)
    ref, margin = P.composite_preint(v, g, *args)
    # what the project's own forward bound (1e-5 max|v|; 2e-5 max|g| for gradients) is worth in this image
    rng = np.random.default_rng(5)
    v2 = v + 1e-5 * np.abs(v).max() * rng.choice([-1.0, 1.0], v.shape)
    g2 = e['g'] + 2e-5 * np.abs(e['g']).max() * rng.choice([-1.0, 1.0], e['g'].shape) if shaded else None
    ref2, _ = P.composite_preint(v2, g2, *args)
    delta = np.abs(ref2 - ref).max()
    out = RR.left_out(margin, 1e-4)
    assert out.sum() <= 0.02 * out.size
    case = dict(values=v.astype(F), grads=None if g is None else g.astype(F), dirs=e['dirs'], t_near=e['tn'], t_far=e['tf'],
                n_steps=n, table=table, v_min=-1.0, v_max=1.0, limit=limit, evaluated=None, steps=n, margin=margin)
    case['ref'], _ = P.composite_preint(case['values'], case['grads'], *args)
    k, ratio = P.tolerance_factor(case, e['step'], ka, kd)
    assert ratio < 4.0
    R_ = e['o'].shape[0]
    want = np.zeros((R_, 4))
    want[hit] = ref
    want[hit, 3] = 1.0 - ref[:, 3]
    err = np.abs(got.astype(np.float64) - want)
    bound = np.full((R_, 1), 4.0 * delta)
    bound[hit, 0] += k * RR.composite_bound(n)
    keep = np.ones(R_, bool)
    keep[hit[out]] = False
    print('render pre-integrated shaded %d: delta %.3e, k %.2f, max err %.3e, max err / bound %.3f, %d of %d rays left out, %d hit, '
          'max opacity %.4f' % (shaded, delta, k, err[keep].max(), (err / bound)[keep].max(), out.sum(), out.size, len(hit),
                                want[:, 3].max()))
    assert len(hit) > 100 and int(n.max()) > 64 and (want[:, 3] >= limit).sum() > 50
    assert (err / bound)[keep].max() <= 1.0
    assert np.array_equal(got[np.setdiff1d(np.arange(R_), hit)], np.zeros((R_ - len(hit), 4), F))
    # a ray's result does not depend on the chunk it sits in
    assert torch.equal(Rn.render_from_net(e['ds'], e['m'], e['o'], e['d'], tf, preintegrated=True, max_samples_per_launch=1 << 11, **kw),
                       image)
    # the default is the midpoint rule, bit for bit
    plain = Rn.render_from_net(e['ds'], e['m'], e['o'], e['d'], tf, **kw)
    assert torch.equal(Rn.render_from_net(e['ds'], e['m'], e['o'], e['d'], tf, preintegrated=False, **kw), plain)
    assert not torch.equal(plain, image)


# ---- 7. empty-space skipping -------------------------------------------------------------------------------------------------

def test_skipping_with_preintegration_stays_within_the_jump_bound(dev):
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    Rn = _render()
    ds = IndexDataset((33, 25, 17), build_index_table=False)
    vol = _t(_half_empty_volume(), dev)
    o, d, _ = _view(dev)
    ranges = Rn.BrickRanges.from_volume(ds, vol, brick=4)
    rng = np.random.default_rng(12)
    table = np.concatenate([rng.uniform(0, 1, (9, 3)), rng.uniform(1, 6, (9, 1))], 1).astype(F)
    table[:4, 3] = 0.0                                                 # no extinction in the rows below 0 (9 rows over [-1, 1])
    tf = Rn.TransferFunction(table)
    plain_stats, stats = {}, {}
    plain = Rn.render_from_volume(ds, vol, o, d, tf, stats=plain_stats, preintegrated=True)
    skipped = Rn.render_from_volume(ds, vol, o, d, tf, stats=stats, skip=ranges, preintegrated=True)
    assert float(plain[:, 3].max()) > 0.3                              # an image, not a blank
    assert stats['skipped_blocks'] > 0 and stats['samples'] < plain_stats['samples']
    step = 1.0 / float(ds.max_dim)
    bound = plain_stats['blocks'] * (1.0 - np.exp(-float(table[:, 3].max()) * step))
    worst = float((skipped.double() - plain.double()).abs().max())
    print('pre-integrated skip: %d blocks skipped, samples %d -> %d, max |skipped - unskipped| %.3e (allowed: %d x %.4f = %.4f)'
          % (stats['skipped_blocks'], plain_stats['samples'], stats['samples'], worst, plain_stats['blocks'],
             bound / plain_stats['blocks'], bound))
    assert worst <= bound
