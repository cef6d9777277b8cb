"""Host-side tests of pre-integrated classification (no GPU): TransferFunction.integral, the float64 restatement
(tests/preint_ref.py) against closed forms and against render_ref.composite, the new C-ABI symbol with the refusals
that are decided before any launch, the CPU refusal, and the conditions and the tolerance the GPU tests rely on."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import preint_ref as P
import render_ref as RR
from latent_feature_grid_compression_amd._lib import LfgcError
from latent_feature_grid_compression_amd.visualization import Render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope='module')
def built_lib():
    from latent_feature_grid_compression_amd.build import build
    return build(verbose=False)


# ---- 1. the integral table ------------------------------------------------------------------------------------------------

def test_integral_is_the_restatement_and_cached():
    rng = np.random.default_rng(8)
    for table in (np.concatenate([rng.uniform(0, 1, (7, 3)), rng.uniform(0, 6, (7, 1))], 1).astype(F),
                  np.array([[0.1, 0.2, 0.3, 4.0], [0.9, 0.8, 0.7, 1.5]], F)):
        tf = Render.TransferFunction(table)
        pre = tf.integral()
        assert pre.dtype == torch.float64 and tuple(pre.shape) == table.shape and pre.is_contiguous()
        want = P.integral(table)
        assert np.array_equal(pre[0].numpy(), np.zeros(4))
        rel = np.abs(pre.numpy() - want)[1:] / np.abs(want)[1:]
        print('K = %d: max relative difference to the restatement %.3e' % (table.shape[0], rel.max()))
        assert rel.max() <= 1e-12
        tau = table[:, 3].astype(np.float64)
        assert np.abs(np.diff(pre[:, 3].numpy()) - 0.5 * (tau[:-1] + tau[1:])).max() <= 1e-12      # trapezoids
        assert tf.integral() is pre
        assert tf.integral_on('cpu') is tf.integral_on('cpu') and torch.equal(tf.integral_on('cpu'), pre)


def test_bracket_is_the_mean_of_the_cell_and_the_lookup_at_a_point():
    rng = np.random.default_rng(9)
    t0, t1 = rng.uniform(0, 2, (5, 4)), rng.uniform(0, 2, (5, 4))
    x0 = rng.uniform(0, 0.6, 5)
    x1 = x0 + rng.uniform(0, 0.4, 5)
    xs = x0[:, None] + (x1 - x0)[:, None] * (np.arange(20001) + 0.5) / 20001          # midpoint quadrature of a cubic
    rgba = t0[:, None, :] + xs[:, :, None] * (t1 - t0)[:, None, :]
    want = np.concatenate([(rgba[..., 3:] * rgba[..., :3]).mean(1), rgba[..., 3:].mean(1)], 1)
    assert np.abs(P.bracket(t0, t1, x0, x1) - want).max() <= 1e-8
    at = t0 + x0[:, None] * (t1 - t0)
    assert np.abs(P.bracket(t0, t1, x0, x0) - np.concatenate([at[:, 3:] * at[:, :3], at[:, 3:]], 1)).max() <= 1e-14


# ---- 2. the linear ramp ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('step', [0.01, 0.04, 0.16, 0.3])
def test_linear_ramp_is_exact_at_any_step(step):
    c = P.ramp_case(step)
    args = (None, c['dirs'], c['t_near'], c['t_far'], c['n_steps'], step, c['table'], -1.0, 1.0, 1.0)
    got, _ = P.composite_preint(c['values'], *args)
    mid, _ = RR.composite(c['values'], *args)
    opacity, mid_opacity = 1.0 - got[:, 3], 1.0 - mid[:, 3]
    print('step %g (%d steps): pre-integrated opacity %.15f, midpoint %.6f, exact %.15f'
          % (step, c['n_steps'][0], opacity[0], mid_opacity[0], c['opacity']))
    assert abs(c['opacity'] - 0.905685) < 1e-6
    assert np.abs(opacity - c['opacity']).max() <= 1e-12
    assert np.abs(got[:, :3] - c['colour'][None, :] * opacity[:, None]).max() <= 1e-6
    if step == 0.16:
        assert np.abs(mid_opacity - c['opacity']).min() > 0.04
    if step == 0.3:
        assert np.abs(mid_opacity - c['opacity']).min() > 0.5


# ---- 3. a constant value: the midpoint rule ----------------------------------------------------------------------------------

@pytest.mark.parametrize('shaded', [False, True])
def test_constant_value_along_a_ray_is_the_midpoint_composite(shaded):
    """Every slab then has the pointwise lookup, and the slabs tile the same chord as the segments do."""
    case = RR.composite_case(1.0, True)
    rng = np.random.default_rng(2)
    R, M = case['values'].shape
    values = np.repeat(rng.uniform(-1.2, 1.2, (R, 1)), M, 1).astype(F)
    n = np.minimum(case['n_steps'], M)                                  # a ray may end early (its last segment is then whole),
    n[:10] = 1                                                          # never late: single-step rays
    n[10:20] = np.minimum(n[10:20], np.arange(2, 12))
    grads = np.repeat(case['grads'][:, :1], M, 1) if shaded else None      # one shade per ray: the colour sums agree too
    args = (values, grads, case['dirs'], case['t_near'], case['t_far'], n, RR.DT, case['table'], -1.0, 1.0, 1.0)
    want, _ = RR.composite(*args)
    got, _ = P.composite_preint(*args)
    print('constant rays: max |pre-integrated - midpoint| %.3e' % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-12


# ---- 4. the library -----------------------------------------------------------------------------------------------------------

def test_new_symbol_is_declared_bound_and_exported(built_lib):
    from latent_feature_grid_compression_amd import _lib, ops
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lfgc.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(lfgc_[a-z0-9_]+)\s*\(', header))
    name = 'lfgc_ray_composite_preint_f32'
    assert name in declared, '%s is not declared in include/lfgc.h' % name
    assert name in _lib.SIGNATURES, '%s has no ctypes signature' % name
    assert hasattr(ctypes.CDLL(built_lib), name), 'liblfgc.so does not export %s' % name
    assert callable(ops.ray_composite_preint)


def test_entry_validates_its_arguments_on_the_host(built_lib):
    """include/lfgc.h's return codes, all decided before anything is launched: no device is touched and no pointer read."""
    from latent_feature_grid_compression_amd import _lib
    lib = _lib.load()
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -4
    a16 = 4096                                    # a 16-byte aligned address that is never read
    names = ('live', 'values', 'grad', 'dirs', 't_near', 't_far', 'n_steps', 'k_next', 'table', 'state', 'pre', 'carry_v', 'carry_k')

    def comp(n_live=10, dt=0.1, S=32, K=7, **ptr):
        p = {k: ptr.get(k, a16) for k in names}
        return lib.lfgc_ray_composite_preint_f32(p['live'], n_live, p['values'], p['grad'], p['dirs'], p['t_near'], p['t_far'],
                                                 p['n_steps'], p['k_next'], dt, S, p['table'], K, -1.0, 3.0, 0.99, 0.3, 0.7,
                                                 p['state'], p['pre'], p['carry_v'], p['carry_k'], None)
    for k in names:
        if k != 'grad':
            assert comp(**{k: None}) == E_NULL, k
    # every refusal comes before the launch, so a call without grad that is refused for another reason shows grad is optional
    assert comp(grad=None, K=1) == E_SHAPE
    assert comp(K=1) == E_SHAPE and comp(K=(1 << 22) + 1) == E_SHAPE
    assert comp(n_live=0) == E_SHAPE and comp(S=16) == E_SHAPE and comp(S=48) == E_SHAPE and comp(dt=0.0) == E_SHAPE
    assert comp(table=a16 + 4) == E_ALIGN and comp(state=a16 + 8) == E_ALIGN and comp(pre=a16 + 8) == E_ALIGN


def test_cpu_tensors_raise_and_a_2d_table_is_refused():
    from latent_feature_grid_compression_amd import ops
    i32, f = torch.zeros(1, dtype=torch.int32), torch.zeros(32)
    tf = Render.TransferFunction(torch.zeros(2, 4))
    with pytest.raises(LfgcError, match='no CPU fallback'):
        ops.ray_composite_preint(i32, f, None, torch.zeros(1, 3), f[:1], f[:1], i32, i32, 0.1, 32, tf.table, tf.integral(), -1.0, 1.0,
                                 0.99, torch.zeros(1, 4), f[:1], i32)
    o, d = Render.pinhole_rays((3, 0, 0), (0, 0, 0), (0, 0, 1), 30, 4, 4)
    with pytest.raises(LfgcError):
        Render.render(lambda p: p[:, 0], o, d, tf, 0.1, [-1, -1, -1], [1, 1, 1], preintegrated=True)
    tf2 = Render.TransferFunction2D(torch.zeros(2, 2, 4), g_max=1.0)
    with pytest.raises(ValueError, match='preintegrated'):
        Render.render(lambda p: (p[:, 0], p), o, d, tf2, 0.1, [-1, -1, -1], [1, 1, 1], preintegrated=True)


# ---- 5. and 6. what the GPU tests rely on -----------------------------------------------------------------------------------

def _slabs(case):
    """(same-cell mask, |u_a - u_b|, cells spanned) of the joined slabs of a case's valid samples."""
    K = case['table'].shape[0]
    u = P.coordinate(case['values'], K, -1.0, 1.0)
    k = np.arange(u.shape[1])[None, :]
    valid = (k < case['n_steps'][:, None]) & case['evaluated']
    joined = valid[:, 1:] & case['evaluated'][:, :-1]
    ua, ub = u[:, :-1][joined], u[:, 1:][joined]
    i_a, _ = P.cell(ua, K)
    i_b, _ = P.cell(ub, K)
    return i_a == i_b, np.abs(ua - ub), np.abs(i_a - i_b)


@pytest.mark.parametrize('jumps', [False, True])
@pytest.mark.parametrize('walk', [False, True])
@pytest.mark.parametrize('shaded', [False, True])
@pytest.mark.parametrize('limit', [0.95, 1.0])
def test_preint_case_is_what_the_gpu_test_needs(limit, shaded, walk, jumps):
    case = P.preint_case(limit, shaded, walk, jumps)
    out = RR.left_out(case['margin'], 1e-5)
    k, ratio = P.tolerance_factor(case)
    print('limit %g shaded %d walk %d jumps %d: %d of %d rays left out; float32 restatement / composite_bound %.3f -> k = %.2f'
          % (limit, shaded, walk, jumps, out.sum(), out.size, ratio, k))
    assert out.sum() <= 0.02 * out.size
    assert ratio < 4.0
    same, du, cells = _slabs(case)
    if walk:
        assert same.mean() > 0.8 and (~same).sum() > 20 and (du < 1e-3).sum() > 20
    else:
        assert same.sum() > 100 and (cells >= 2).sum() > 100
    if limit < 1.0:
        assert ((1 - case['ref'][:, 3]) >= limit).sum() >= 10
    if jumps:
        S, n = case['S'], case['n_steps']
        assert (n[0::P.JUMP_EVERY] > S).sum() >= 10                      # rays that lose samples, and their closing half
        assert (n[1::P.JUMP_EVERY] > S).sum() >= 10                      # rays that open again behind a jump
        plain = P.preint_case(limit, shaded, walk, False)
        assert np.abs(plain['ref'] - case['ref'])[1::P.JUMP_EVERY].max() > 1e-3      # the jump shows
        if limit == 1.0:                                                 # (under 0.95 most rays are opaque after a block)
            assert np.abs(plain['ref'] - case['ref'])[0::P.JUMP_EVERY].max() > 1e-3
        assert np.array_equal(plain['ref'][2::P.JUMP_EVERY], case['ref'][2::P.JUMP_EVERY])
