"""Host-side tests of the isosurface ray caster (no GPU): the NumPy restatement (tests/iso_ref.py) against closed forms,
the new C entries in the header and the binding, the argument checks that run before any launch, and the two pure-torch
functions (shade_isosurface, surface_deviation) on hand-made hits."""
import math
import os
import re

import numpy as np
import pytest
import torch

import iso_ref as IR
import render_ref as RR
from latent_feature_grid_compression_amd import _lib, ops
from latent_feature_grid_compression_amd._lib import LfgcError
from latent_feature_grid_compression_amd.visualization import Render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('lfgc_ray_iso_scan_f32', 'lfgc_ray_iso_refine_f32', 'lfgc_ray_iso_finish_f32')


# ---- the restatement against mathematics -------------------------------------------------------------------------------

def _f32_of(fn64):
    """A value function for IR.march: float64 closed form of the float32 positions, rounded to float32."""
    return lambda p: fn64(np.asarray(p, np.float64)).astype(np.float32)


@pytest.mark.parametrize('refine_steps', [0, 3])
def test_linear_field_along_a_ray_is_found_by_the_secant_step(refine_steps):
    """v = g.p + c is linear along every ray, so the secant step lands on the root whatever the bracket: with NO bisection
    the depth is already exact up to float32 rounding -- 8 2^-24 max(1, t) for t and the positions, plus the rounding of
    the two float32 end values (2^-24 |v| each, |v| <= 2 here) carried to t by the slope |g.d|: 4 2^-24 * 2 / |g.d|."""
    g, c, iso = np.array([0.7, -0.4, 0.5]), 0.05, 0.2
    o, d = RR.ray_set()
    with np.errstate(all='ignore'):
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[~np.isfinite(d).all(1)] = 0
    res = IR.march(_f32_of(lambda p: p @ g + c), o, d, iso, RR.DT, RR.BOX, refine_steps)
    o64, d64 = o.astype(np.float64), d.astype(np.float64)
    slope = d64 @ g
    with np.errstate(all='ignore'):
        t_true = (iso - c - o64 @ g) / slope
    # rays whose crossing is at least a step inside their chord, with a slope that keeps the bound meaningful
    tn, tf = res['tn'].astype(np.float64), res['tf'].astype(np.float64)
    sure = (res['n'] > 2) & (np.abs(slope) > 0.1) & (t_true > tn + RR.DT) & (t_true < tf - RR.DT)
    assert sure.sum() > 100
    assert res['hit'][sure].all()
    err = np.abs(res['t'][sure].astype(np.float64) - t_true[sure])
    bound = 8 * 2.0 ** -24 * np.maximum(1.0, t_true[sure]) + 8 * 2.0 ** -24 / np.abs(slope[sure])
    assert (err <= bound).all(), (err / bound).max()
    # the surface does not pass through the chord at all: a miss, t = inf
    clear = (res['n'] > 0) & ((t_true < tn - RR.DT) | (t_true > tf + RR.DT))
    assert clear.sum() > 20 and not res['hit'][clear].any() and np.isinf(res['t'][clear]).all()
    assert not res['hit'][res['n'] == 0].any()
    # the bracket: ordered, holds t, no wider than the step halved refine_steps times (+ an ulp of t per rounded midpoint)
    h = res['hit']
    assert (res['t_lo'][h] <= res['t'][h]).all() and (res['t'][h] <= res['t_hi'][h]).all()
    width = res['t_hi'][h].astype(np.float64) - res['t_lo'][h]
    assert (width <= RR.DT * 2.0 ** -refine_steps + 2 * np.spacing(res['t_hi'][h])).all()


def test_plane_depth_is_within_the_bisection_bound():
    """The plane x = 0.25 through the unit box, seen by the sphere tests' two ray sets: |t - t_true| <= dt 2^-8 + rounding;
    both directions of the sign change count (the orthographic set looks at the plane from the other side)."""
    dt, n_ref = IR.SPHERE_DT, 8
    for which, iso in (('pinhole', 0.25), ('ortho', 0.25)):
        o, d = IR.sphere_rays(which)
        res = IR.march(_f32_of(lambda p: p[:, 0]), o, d, iso, dt, IR.BOX1, n_ref)
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        t_true = (iso - o64[:, 0]) / d64[:, 0]
        sure = (res['n'] > 2) & (t_true > res['tn'] + dt) & (t_true < res['tf'] - dt)
        assert sure.sum() > 400 and res['hit'][sure].all()
        err = np.abs(res['t'][sure] - t_true[sure])
        assert (err <= IR.depth_bound(dt, n_ref, t_true[sure])).all()
        assert np.abs(res['position'][sure][:, 0] - iso).max() <= 1e-6
        clear = (res['n'] == 0) | (t_true < res['tn'] - dt) | (t_true > res['tf'] + dt)
        assert clear.sum() > 100 and not res['hit'][clear].any()
    # entering (pinhole: the eye is at x > 0.25, the set {x >= 0.25} is left) and leaving both happened
    assert IR.sphere_rays('pinhole')[1][:, 0].max() < 0 < IR.sphere_rays('ortho')[1][:, 0].min()


@pytest.mark.parametrize('which', ['pinhole', 'ortho'])
def test_sphere_depth_is_within_the_bisection_bound(which):
    """v = r - |p - c|, iso 0: the GPU test's case through the restatement alone.  Rays with impact parameter b > r miss,
    rays with b < sqrt(r^2 - dt^2) hit within the bound; the grazing band in between is at most 2 % of the hitting rays."""
    dt, n_ref, r, c = IR.SPHERE_DT, 8, IR.SPHERE_R, IR.SPHERE_C
    o, d = IR.sphere_rays(which)
    res = IR.march(_f32_of(lambda p: r - np.linalg.norm(p - c, axis=1)), o, d, 0.0, dt, IR.BOX1, n_ref)
    b, t_true, _ = IR.sphere_truth(o, d)
    sure = b < math.sqrt(r * r - dt * dt)
    assert sure.sum() > 300 and (b > r).sum() > 300
    assert not res['hit'][b > r].any()
    assert res['hit'][sure].all()
    assert (np.abs(res['t'][sure] - t_true[sure]) <= IR.depth_bound(dt, n_ref, t_true[sure])).all()
    assert ((b < r) & ~sure).sum() <= 0.02 * (b < r).sum()


def test_scan_restatement_rules():
    """One ray by hand: sample 0 never crosses, the carry is used across blocks only when k_next > 0, padding never crosses,
    v == iso is inside, a NaN is not."""
    tn, tf, n = np.array([1.0], np.float32), np.array([1.5], np.float32), np.array([5], np.int32)
    iso, dt = 0.5, 0.1

    def run(values, k0=0, carry=0.0):
        state, bracket, k_next = IR.new_state(1)
        state[0, 0], k_next[0] = carry, k0
        return IR.scan([0], np.array([values], np.float32), tn, tf, n, k_next, dt, iso, state, bracket)
    st, br, kn = run([0, 0, 1, 0, 0, 1, 1, 1])                 # two crossings: the first wins
    assert kn[0] == 2 and st[0, 3] == 0 and st[0, 0] == 1
    assert np.array_equal(br[0], np.array([IR.t_mid(tn, tf, 1, dt)[0], IR.t_mid(tn, tf, 2, dt)[0], -0.5, 0.5], np.float32))
    st, br, kn = run([0, 0, 0, 0, 0, 1, 1, 1])                 # only in padding (n = 5): no hit
    assert kn[0] == 8 and st[0, 3] == 1 and st[0, 0] == 1
    st, br, kn = run([0, 0, 0, 0, 0, 0, 0, 0], carry=1.0)      # k_next = 0: the carry is not a predecessor
    assert st[0, 3] == 1
    st, br, kn = run([0, 0, 0, 0], k0=1, carry=1.0)            # k_next > 0: it is
    assert kn[0] == 1 and st[0, 3] == 0 and br[0, 2] == np.float32(0.5) and br[0, 3] == np.float32(-0.5)
    st, br, kn = run([0, 0.5, 0.5, 0.5, 0.5, 0, 0, 0])         # v == iso is inside: a crossing at sample 1 with f_hi = 0
    assert kn[0] == 1 and br[0, 3] == 0
    st, br, kn = run([1, 1, np.nan, 1, 1, 1, 1, 1])            # a NaN is outside
    assert kn[0] == 2 and np.isnan(br[0, 3])
    # refine with a NaN end keeps going, finish takes the midpoint of such a bracket
    o, d = np.zeros((1, 3), np.float32), np.array([[1.0, 0, 0]], np.float32)
    t, p = IR.finish([0], o, d, br)
    assert t[0] == np.float32(0.5) * (br[0, 0] + br[0, 1]) and p[0, 0] == t[0]


# ---- header and binding ---------------------------------------------------------------------------------------------------

def test_entries_are_declared_and_bound_with_matching_arity():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lfgc.h')).read(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, '%s is not declared in include/lfgc.h' % name
        params = [p for p in m.group(1).split(',') if p.strip()]
        assert name in _lib.SIGNATURES, '%s is not bound in _lib.py' % name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib.c_int and len(argtypes) == len(params), (name, len(argtypes), len(params))
        assert params[-1].split()[0] == 'lfgc_stream_t'
    for fn in ('ray_iso_scan', 'ray_iso_refine', 'ray_iso_finish'):
        assert callable(getattr(ops, fn))
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in text for name in ENTRIES)


def test_library_exports_the_entries():
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        getattr(lib, name)


# ---- argument checks, all before any launch --------------------------------------------------------------------------------

def _cpu_rays():
    return Render.pinhole_rays((3, 0, 0), (0, 0, 0), (0, 0, 1), 30, 4, 4)


def test_isosurface_arguments_are_checked_before_any_launch():
    o, d = _cpu_rays()
    box = ([-1, -1, -1], [1, 1, 1])
    fn = lambda p: p[:, 0]                                      # noqa: E731
    for bad in (float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError):
            Render.isosurface(fn, o, d, bad, 0.1, *box)
    for bad in (-1, 1.5, 65):
        with pytest.raises(ValueError):
            Render.isosurface(fn, o, d, 0.0, 0.1, *box, refine_steps=bad)
    for bad in (0, 16, 48):
        with pytest.raises(ValueError):
            Render.isosurface(fn, o, d, 0.0, 0.1, *box, block_steps=bad)
    with pytest.raises(ValueError):
        Render.isosurface(fn, o, d, 0.0, 0.0, *box)
    for bad in (-1.0, 1.0, 1.5, float('nan')):                  # outside the open clamp range of the eval-mode output
        with pytest.raises(ValueError):
            Render.isosurface_from_net([1.0, 1.0, 1.0], torch.nn.Identity(), o, d, bad, step=0.1)


def test_cpu_tensors_raise():
    o, d = _cpu_rays()
    with pytest.raises(LfgcError):
        Render.isosurface(lambda p: p[:, 0], o, d, 0.0, 0.1, [-1, -1, -1], [1, 1, 1])
    with pytest.raises(LfgcError):
        Render.isosurface_from_net([1.0, 1.0, 1.0], torch.nn.Identity(), o, d, 0.0, step=0.1)
    i32, f4 = torch.zeros(16, dtype=torch.int32), torch.zeros(16, 4)
    f1 = torch.zeros(16)
    with pytest.raises(LfgcError):
        ops.ray_iso_scan(i32, torch.zeros(16 * 32), f1, f1, i32, i32, 0.1, 32, 0.0, f4, f4)
    with pytest.raises(LfgcError):
        ops.ray_iso_refine(i32, None, o, d, 0.0, f4)
    with pytest.raises(LfgcError):
        ops.ray_iso_finish(i32, o, d, f4)


# ---- shading and the deviation measure on hand-made hits -------------------------------------------------------------------

def _hits(hit, t, normal):
    hit = torch.tensor(hit, dtype=torch.bool)
    t = torch.tensor(t, dtype=torch.float32)
    normal = torch.tensor(normal, dtype=torch.float32)
    z = torch.zeros(len(hit))
    return Render.IsoHits(hit, t, torch.zeros(len(hit), 3), normal, z, t, t)


def test_shade_isosurface_on_hand_made_hits():
    s = math.sqrt(0.5)
    inf = float('inf')
    hits = _hits([True, True, False, True], [1.0, 2.0, inf, 3.0], [[0, 0, -1.0], [0, -s, -s], [0, 0, 0], [0, 0, 0]])
    dirs = torch.tensor([[0, 0, 2.0]] * 4)                          # not unit: normalised by the function
    img = Render.shade_isosurface(hits, dirs, colour=(1.0, 0.5, 0.25), ka=0.2, kd=0.6, ks=0.1, shininess=2.0)
    assert img.shape == (4, 4)
    c = [1.0, s, 0.0, 0.0]
    for i in (0, 1, 3):
        lum = 0.2 + 0.6 * c[i]
        want = [1.0 * lum + 0.1 * c[i] ** 2, 0.5 * lum + 0.1 * c[i] ** 2, 0.25 * lum + 0.1 * c[i] ** 2, 1.0]
        assert np.allclose(img[i].numpy(), want, rtol=0, atol=1e-6)
    assert torch.equal(img[2], torch.zeros(4))                      # a miss: transparent
    # defaults: white, ka 0.3, kd 0.7, no highlight -> the render's headlight; and it composes with background()
    img = Render.shade_isosurface(hits, dirs)
    assert np.allclose(img[:, 0].numpy(), [1.0, 0.3 + 0.7 * s, 0.0, 0.3], rtol=0, atol=1e-6)
    over = Render.background(img, (0.0, 0.0, 1.0))
    assert np.allclose(over[2].numpy(), [0, 0, 1]) and np.allclose(over[0].numpy(), [1, 1, 1])
    with pytest.raises(ValueError):
        Render.shade_isosurface(hits, dirs[:3])


def test_surface_deviation_on_hand_made_hits():
    s = math.sqrt(0.5)
    inf = float('inf')
    a = _hits([True, True, True, False, False], [1.0, 2.0, 3.0, inf, inf],
              [[0, 0, -1.0], [0, 0, -1.0], [0, 0, -1.0], [0, 0, 0], [0, 0, 0]])
    b = _hits([True, True, False, True, False], [1.5, 2.0, inf, 1.0, inf],
              [[0, -1.0, 0], [0, -s, -s], [0, 0, 0], [0, 0, -1.0], [0, 0, 0]])
    dev_ = Render.surface_deviation(a, b)
    assert dev_['mismatch'] == 2 / 5 and dev_['common'] == 2
    assert abs(dev_['depth_rms'] - math.sqrt(0.125)) <= 1e-7 and abs(dev_['depth_max'] - 0.5) <= 1e-7
    assert abs(dev_['angle_max'] - 90.0) <= 1e-4 and abs(dev_['angle_mean'] - 67.5) <= 1e-4
    same = Render.surface_deviation(a, a)
    assert same == {'mismatch': 0.0, 'common': 3, 'depth_rms': 0.0, 'depth_max': 0.0, 'angle_mean': 0.0, 'angle_max': 0.0}
    none = Render.surface_deviation(_hits([False], [inf], [[0, 0, 0]]), _hits([True], [1.0], [[0, 0, -1.0]]))
    assert none['mismatch'] == 1.0 and none['common'] == 0 and none['depth_max'] == 0.0
    with pytest.raises(ValueError):
        Render.surface_deviation(a, _hits([True], [1.0], [[0, 0, -1.0]]))


# ---- conditions the GPU tests rely on, checked here on the CPU -----------------------------------------------------------

@pytest.mark.parametrize('S', [32, 64])
def test_scan_case_covers_the_places_a_crossing_can_sit(S):
    case = IR.scan_case(S)
    live, n = case['live'], case['n_steps']
    tags = case['tags'][live]
    for tag in IR.SCAN_PATTERNS:
        assert (tags == tag).sum() >= 2, tag
    assert n[live[0]] == 1 and n[live[1]] == 2
    state, bracket, k_next, lists = IR.scan_chain(case, live)
    assert len(lists[1]) < len(lists[0]) and len(lists[2]) > 0          # rays drop out, some march through all three blocks
    hit = state[:, 3] == 0
    want = case['expect']
    assert np.array_equal(hit[live], want[live] >= 0)
    assert np.array_equal(k_next[live][hit[live]], want[live][hit[live]])
    pad = live[tags == 'padding']
    assert not hit[pad].any() and (n[pad] % S != 0).all()
    assert hit[live[1]] and not hit[live[0]]
    eq = live[tags == 'equal']
    assert (bracket[eq, 3] == 0).all() and (bracket[eq, 2] == np.float32(-1.25)).all()
    assert np.isnan(bracket[live[tags == 'nan'], 3]).all()
    both = live[tags == 'block_first']
    assert (k_next[both] == S).all() and hit[both].all()                 # found through the carry, in the second call
    # brackets are the two sample midpoints around the crossing
    r = live[hit[live]]
    assert np.array_equal(bracket[r, 0], IR.t_mid(case['t_near'][r], case['t_far'][r], k_next[r] - 1, RR.DT))
    assert np.array_equal(bracket[r, 1], IR.t_mid(case['t_near'][r], case['t_far'][r], k_next[r], RR.DT))
