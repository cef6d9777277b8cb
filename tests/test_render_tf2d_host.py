"""Host-side tests of the 2-D transfer functions (no GPU): TransferFunction2D's validation, its value projection and
the boundary-emphasis ramp on hand-made tables, the two new C-ABI symbols, the argument errors that are decided before
any launch, the CPU refusal, and the float64 restatement (tests/tf2d_ref.py) against render_ref.composite."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import render_ref as RR
import tf2d_ref as T2
from latent_feature_grid_compression_amd._lib import LfgcError
from latent_feature_grid_compression_amd.visualization import Render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('lfgc_ray_composite2d_f32', 'lfgc_joint_histogram_f32')


@pytest.fixture(scope='module')
def built_lib():
    from latent_feature_grid_compression_amd.build import build
    return build(verbose=False)


def _good():
    return np.array([[[0, 0, 0, 0.0], [0.1, 0.2, 0.3, 1.0], [0, 0, 0, 0.5]],
                     [[1, 1, 1, 2.0], [0.5, 0.5, 0.5, 0.0], [1, 0, 1, 3.0]]], np.float32)          # (2, 3, 4)


# ---- the class ------------------------------------------------------------------------------------------------------------

def test_transfer_function_2d_validation():
    tf = Render.TransferFunction2D(_good(), g_max=4.0)
    assert tf.table.shape == (2, 3, 4) and tf.table.dtype == torch.float32 and tf.table.is_contiguous()
    assert (tf.v_min, tf.v_max, tf.g_max) == (-1.0, 1.0, 4.0)
    assert tf.on('cpu') is tf.on('cpu')
    bad_tables = [_good()[:1],                                      # Kv < 2
                  _good()[:, :1],                                   # Kg < 2
                  _good()[..., :3],                                 # not (Kv, Kg, 4)
                  _good()[0]]                                       # a 1-D table
    for t in bad_tables:
        with pytest.raises(ValueError):
            Render.TransferFunction2D(t, g_max=1.0)
    neg, nan = _good(), _good()
    neg[1, 2, 3] = -0.1
    nan[0, 1, 0] = np.nan
    for t in (neg, nan):
        with pytest.raises(ValueError):
            Render.TransferFunction2D(t, g_max=1.0)
    with pytest.raises(ValueError):
        Render.TransferFunction2D(_good(), v_min=0.5, v_max=0.5, g_max=1.0)
    for g_max in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError):
            Render.TransferFunction2D(_good(), g_max=g_max)


def test_value_projection_takes_the_largest_extinction_of_a_row():
    tf = Render.TransferFunction2D(_good(), v_min=-0.5, v_max=0.75, g_max=4.0)
    p = tf.value_projection()
    assert isinstance(p, Render.TransferFunction) and p.table.shape == (2, 4)
    assert (p.v_min, p.v_max) == (-0.5, 0.75)
    assert torch.equal(p.table[:, 3], torch.tensor([1.0, 3.0]))
    assert bool(torch.isfinite(p.table).all())
    assert tf.value_projection() is p                                # cached: BrickRanges caches its tables by identity
    clear = _good()
    clear[0, :, 3] = 0.0
    assert torch.equal(Render.TransferFunction2D(clear, g_max=1.0).value_projection().table[:, 3], torch.tensor([0.0, 3.0]))


def test_from_ramp_keeps_the_colours_and_ramps_the_extinction():
    tf = Render.TransferFunction([[0.1, 0.2, 0.3, 4.0], [0.9, 0.8, 0.7, 0.0], [0.5, 0.5, 0.5, 2.0]], v_min=0.0, v_max=2.0)
    t2 = Render.TransferFunction2D.from_ramp(tf, 1.0, 3.0, 5, 4.0)         # g rows at 0, 1, 2, 3, 4: ramp 0, 0, 0.5, 1, 1
    assert t2.table.shape == (3, 5, 4) and (t2.v_min, t2.v_max, t2.g_max) == (0.0, 2.0, 4.0)
    for j in range(5):
        assert torch.equal(t2.table[:, j, :3], tf.table[:, :3])
    ramp = torch.tensor([0.0, 0.0, 0.5, 1.0, 1.0])
    assert torch.equal(t2.table[..., 3], tf.table[:, 3:4] * ramp.view(1, 5))
    assert torch.equal(t2.value_projection().table[:, 3], tf.table[:, 3])
    assert Render.TransferFunction2D.from_ramp(tf, 0.0, 2.0, 2).g_max == 2.0          # g_max defaults to g_hi
    for args in ((2.0, 1.0, 5, 4.0), (1.0, 1.0, 5, 4.0), (-1.0, 1.0, 5, 4.0), (1.0, 3.0, 1, 4.0), (1.0, 3.0, 5, 0.0)):
        with pytest.raises(ValueError):
            Render.TransferFunction2D.from_ramp(tf, *args)


# ---- the library ----------------------------------------------------------------------------------------------------------

def test_new_symbols_are_declared_bound_and_exported(built_lib):
    from latent_feature_grid_compression_amd import _lib, ops
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lfgc.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(lfgc_[a-z0-9_]+)\s*\(', header))
    lib = ctypes.CDLL(built_lib)
    for name in NEW_SYMBOLS:
        assert name in declared, '%s is not declared in include/lfgc.h' % name
        assert name in _lib.SIGNATURES, '%s has no ctypes signature' % name
        assert hasattr(lib, name), 'liblfgc.so does not export %s' % name
    assert callable(ops.ray_composite2d) and callable(ops.joint_histogram)
    assert callable(Render.joint_histogram_from_net) and callable(Render.joint_histogram_from_volume)


def test_entries_validate_their_arguments_on_the_host(built_lib):
    """include/lfgc.h's return codes, all decided before anything is launched: no device is touched and no pointer read."""
    from latent_feature_grid_compression_amd import _lib
    lib = _lib.load()
    OK, E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = 0, -1, -2, -3, -4
    a16 = 4096                                    # a 16-byte aligned address that is never read
    names = ('live', 'values', 'grad', 'dirs', 't_near', 't_far', 'n_steps', 'k_next', 'table', 'state')

    def comp(n_live=10, dt=0.1, S=32, Kv=7, Kg=5, g_scale=2.0, shade=0, **ptr):
        p = {k: ptr.get(k, a16) for k in names}
        return lib.lfgc_ray_composite2d_f32(p['live'], n_live, p['values'], p['grad'], p['dirs'], p['t_near'], p['t_far'], p['n_steps'],
                                            p['k_next'], dt, S, p['table'], Kv, Kg, -1.0, 3.0, g_scale, shade, 0.99, 0.3, 0.7,
                                            p['state'], None)
    for k in names:
        assert comp(**{k: None}) == E_NULL, k                           # grad included: it is required
    assert comp(Kv=1) == E_SHAPE and comp(Kg=1) == E_SHAPE
    assert comp(Kv=2048, Kg=2049) == E_SHAPE                            # Kv * Kg > 2^22
    for g_scale in (0.0, -1.0, float('inf'), float('nan')):
        assert comp(g_scale=g_scale) == E_SHAPE
    assert comp(shade=2) == E_SHAPE
    assert comp(n_live=0) == E_SHAPE and comp(S=16) == E_SHAPE and comp(S=48) == E_SHAPE and comp(dt=0.0) == E_SHAPE
    assert comp(table=a16 + 4) == E_ALIGN and comp(state=a16 + 8) == E_ALIGN

    def hist(values=a16, grad=a16, n=10, Bv=8, Bg=5, v_min=-1.0, v_scale=4.0, g_scale=2.5, counts=a16):
        return lib.lfgc_joint_histogram_f32(values, grad, n, Bv, Bg, v_min, v_scale, g_scale, counts, None)
    assert hist(values=None) == E_NULL and hist(grad=None) == E_NULL and hist(counts=None) == E_NULL
    assert hist(n=-1) == E_SHAPE and hist(Bv=0) == E_SHAPE and hist(Bg=0) == E_SHAPE
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        assert hist(v_scale=bad) == E_SHAPE and hist(g_scale=bad) == E_SHAPE
    assert hist(v_min=float('nan')) == E_SHAPE
    assert hist(Bv=128, Bg=129) == E_UNSUPPORTED                        # more than 16384 bins: 64 KB of LDS
    assert hist(counts=a16 + 4) == E_ALIGN
    assert hist(n=0) == OK and hist(n=0, Bv=128, Bg=128) == OK          # nothing to do: LFGC_OK at once


def test_cpu_tensors_raise():
    from latent_feature_grid_compression_amd import ops
    i32, f = torch.zeros(1, dtype=torch.int32), torch.zeros(32)
    table = torch.zeros(2, 2, 4)
    with pytest.raises(LfgcError, match='no CPU fallback'):
        ops.ray_composite2d(i32, f, torch.zeros(32, 3), torch.zeros(1, 3), f[:1], f[:1], i32, i32, 0.1, 32, table, -1.0, 1.0, 1.0,
                            0.99, torch.zeros(1, 4))
    with pytest.raises(LfgcError, match='no CPU fallback'):
        ops.joint_histogram(f, torch.zeros(32, 3), (4, 4), -1.0, 1.0, 1.0)
    o, d = Render.pinhole_rays((3, 0, 0), (0, 0, 0), (0, 0, 1), 30, 4, 4)
    tf = Render.TransferFunction2D(_good(), g_max=1.0)
    with pytest.raises(LfgcError):
        Render.render(lambda p: (p[:, 0], p), o, d, tf, 0.1, [-1, -1, -1], [1, 1, 1])


# ---- the restatement ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shaded', [False, True])
@pytest.mark.parametrize('Kg', [2, 5])
def test_a_table_constant_along_g_is_the_1d_composite(Kg, shaded):
    """In float64 the 2-D composite of a table repeated along g IS render_ref.composite of the 1-D table: lo == hi, so the
    lerp along g adds h * 0."""
    case = RR.composite_case(0.95, True)
    table2 = np.repeat(case['table'][:, None, :], Kg, 1)
    args = (case['dirs'], case['t_near'], case['t_far'], case['n_steps'], RR.DT)
    want, wm = RR.composite(case['values'], case['grads'] if shaded else None, *args, case['table'], -1.0, 1.0, 0.95)
    got, gm = T2.composite2d(case['values'], case['grads'], *args, table2, -1.0, 1.0, T2.G_MAX, 0.95, shaded)
    assert np.abs(got - want).max() == 0.0 and np.array_equal(gm, wm)


def test_lookup_at_the_rows_and_outside_the_range():
    rng = np.random.default_rng(3)
    table = rng.uniform(0, 1, (4, 3, 4))
    # at the rows themselves: v = -1 + 2 i / 3 (exact for i = 0, 3), |g| = j
    got = T2.lookup2d(table, np.array([-1.0, 1.0, -1.0, 1.0]), np.array([0.0, 0.0, 2.0, 1.0]), -1.0, 1.0, 2.0)
    # (a + 1 * (b - a) is b up to one rounding)
    assert np.allclose(got, np.stack([table[0, 0], table[3, 0], table[0, 2], table[3, 1]]), rtol=0, atol=1e-15)
    # outside: the end rows; a NaN: row 0 of its axis
    got = T2.lookup2d(table, np.array([-7.0, 9.0, np.nan, 1.0]), np.array([5.0, np.inf, 0.0, np.nan]), -1.0, 1.0, 2.0)
    assert np.allclose(got, np.stack([table[0, 2], table[3, 2], table[0, 0], table[3, 0]]), rtol=0, atol=1e-15)
    # the middle of a cell is the mean of its four corners
    got = T2.lookup2d(table, np.array([0.0]), np.array([0.5]), -1.0, 1.0, 2.0)
    assert np.allclose(got[0], table[1:3, 0:2].mean((0, 1)), rtol=0, atol=1e-15)


@pytest.mark.parametrize('shaded', [False, True])
@pytest.mark.parametrize('limit', [0.95, 1.0])
def test_composite_case2d_is_what_the_gpu_test_needs(limit, shaded):
    """The conditions the GPU test relies on: at most 2 % of the rays decided within 1e-5 of the limit, both clamps of the
    g axis and zero gradients present, and a table that does depend on g."""
    case = T2.composite_case2d(limit, shaded)
    out = RR.left_out(case['margin'], 1e-5)
    print('limit %g shaded %d: %d of %d rays left out' % (limit, shaded, out.sum(), out.size))
    assert out.sum() <= 0.02 * out.size
    assert case['table'].shape == (7, 5, 4) and case['table'].dtype == np.float32
    gn = np.sqrt((case['grads'].astype(np.float64) ** 2).sum(2))
    assert 0.2 < (gn > case['g_max']).mean() < 0.3 and 0.08 < (gn == 0).mean() < 0.12
    assert (np.abs(case['values']) > 1.0).mean() > 0.1
    flat, _ = RR.composite(case['values'], case['grads'] if shaded else None, case['dirs'], case['t_near'], case['t_far'],
                           case['n_steps'], RR.DT, case['table'][:, 0], -1.0, 1.0, limit)
    assert np.abs(flat - case['ref']).max() > 1e-2                   # the g axis shows
    if limit < 1.0:
        assert ((1 - case['ref'][:, 3]) >= limit).sum() >= 10


def test_histogram_restatement_on_hand_made_samples():
    v = np.array([-1.5, -1.0, -0.5, 0.0, 0.999, 1.0, 3.0, np.nan], np.float32)
    g = np.zeros((8, 3), np.float32)
    g[:, 0] = [0.0, 0.5, 1.0, 1.999, 2.0, 7.0, np.nan, 0.0]
    i, j = T2.histogram_bins(v, g, (4, 2), -1.0, 1.0, 2.0)
    assert i.tolist() == [0, 0, 1, 2, 3, 3, 3, 0] and j.tolist() == [0, 0, 1, 1, 1, 1, 0, 0]
    h = T2.histogram(v, g, (4, 2), -1.0, 1.0, 2.0)
    assert h.sum() == 8 and h.shape == (4, 2) and h[0, 0] == 3
