"""Host-side tests of the renderer (no GPU): the NumPy restatement against closed forms, the ray generators, the
transfer function's validation, the CPU refusal, and the CPU-side conditions the GPU tests rely on."""
import math

import numpy as np
import pytest
import torch

import render_ref as RR
from latent_feature_grid_compression_amd._lib import LfgcError
from latent_feature_grid_compression_amd.visualization import Render


# ---- the restatement against mathematics -------------------------------------------------------------------------------

def _march(origins, dirs, box, dt, table, v_min, v_max, value_of, limit=1.0):
    """Render with the restatement alone: every step of every ray, values from value_of(positions)."""
    o, d = np.asarray(origins, np.float32), np.asarray(dirs, np.float32)
    diag = float(np.linalg.norm(np.asarray(box[1], np.float64) - np.asarray(box[0], np.float64)))
    tn, tf, n = RR.clip(o, d, box[0], box[1], 0.0, np.inf, dt, max(32, int(math.ceil(2 * diag / dt))))
    M = int(n.max())
    live = np.arange(o.shape[0])
    pos, _ = RR.samples(live, o, d, tn, tf, n, np.zeros(o.shape[0], np.int32), dt, M)
    values = value_of(pos.astype(np.float64)).reshape(o.shape[0], M)
    st, _ = RR.composite(values, None, d, tn, tf, n, dt, table, v_min, v_max, limit)
    return st, (tn, tf, n)


_CHORD_RAYS = [((-3.0, 0.1, 0.2), (1.0, 0.0, 0.0), 2.0),          # through the x faces of +-(1, 0.75, 0.5): chord 2
               ((0.3, 2.0, -0.1), (0.0, -1.0, 0.0), 1.5),          # y faces: 1.5
               ((0.3, 0.2, -4.0), (0.0, 0.0, 1.0), 1.0),           # z faces: 1
               ((-2.0, -1.5, -1.0), tuple(np.array([2.0, 1.5, 1.0]) / math.sqrt(7.25)), math.sqrt(7.25))]   # the diagonal


@pytest.mark.parametrize('dt', [0.0371, 0.25, 0.013, 3.0])
def test_constant_medium_is_exact_for_any_step(dt):
    """Constant extinction sigma and colour c over a chord L: opacity 1 - exp(-sigma L), colour c (1 - exp(-sigma L)),
    whatever the step -- the short last segment makes the segment lengths add up to the chord."""
    sigma, c = 1.7, np.array([0.9, 0.5, 0.2])
    table = np.tile(np.array([*c, sigma]), (2, 1))
    o = np.array([r[0] for r in _CHORD_RAYS], np.float32)
    d = np.array([r[1] for r in _CHORD_RAYS], np.float32)
    st, (tn, tf, n) = _march(o, d, RR.BOX, dt, table, -1.0, 1.0, lambda p: np.zeros(p.shape[0]))
    L = tf.astype(np.float64) - tn.astype(np.float64)            # the chord the float32 clip found ...
    assert np.allclose(L, [r[2] for r in _CHORD_RAYS], rtol=0, atol=1e-6)      # ... is the geometric one
    want = 1.0 - np.exp(-sigma * L)
    assert np.abs((1.0 - st[:, 3]) - want).max() <= 1e-12
    assert np.abs(st[:, :3] - want[:, None] * c[None]).max() <= 1e-12


def test_float32_segments_cover_the_chord():
    """The float32 segments the kernels form: the first starts at t_near, the last ends at t_far, and since a_k is never an
    accumulated sum, neighbours meet to within an ulp of t however many steps there are."""
    o, d = RR.ray_set()
    tn, tf, n = RR.clip(o, d, RR.BOX[0], RR.BOX[1], 0.0, np.inf, RR.DT, RR.ray_max_steps())
    hit = np.nonzero((n > 0) & (n < RR.ray_max_steps()))[0]
    assert len(hit) > 300
    for r in hit[::7]:
        k = np.arange(n[r])
        a, b = RR.segments(np.full(n[r], tn[r]), np.full(n[r], tf[r]), k, RR.DT)
        assert b[-1] == tf[r] and a[0] == tn[r]
        assert n[r] == 1 or np.abs(a[1:].astype(np.float64) - b[:-1].astype(np.float64)).max() <= 2.0 ** -22 * max(1.0, abs(float(tf[r])))
        assert np.all(b >= a)


def test_two_slab_medium_matches_the_two_segment_formula():
    """Table with a jump in the middle of the value range, a volume whose value is -1 for x < 0 and +1 for x > 0, rays
    along x: two homogeneous segments.  A step that puts a sample boundary on x = 0 keeps every sample inside one slab."""
    s1, c1, s2, c2 = 0.8, np.array([1.0, 0.2, 0.1]), 2.5, np.array([0.1, 0.3, 1.0])
    # K = 4 over [-1, 1]: rows at -1, -1/3, 1/3, 1 -- values -1 and +1 sit on the first and the last row
    table = np.array([[*c1, s1], [*c1, s1], [*c2, s2], [*c2, s2]])
    o = np.array([[-3.0, 0.1, 0.2], [-2.0, -0.3, 0.4]], np.float32)
    d = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]], np.float32)
    for dt in (0.25, 0.125, 0.0625):                               # powers of two: x = 0 is a segment boundary, exactly
        st, _ = _march(o, d, RR.BOX, dt, table, -1.0, 1.0, lambda p: np.where(p[:, 0] < 0, -1.0, 1.0))
        e1, e2 = math.exp(-s1 * 1.0), math.exp(-s2 * 1.0)
        rgb = c1 * (1 - e1) + e1 * c2 * (1 - e2)
        assert np.abs(st[:, :3] - rgb[None]).max() <= 1e-12
        assert np.abs(st[:, 3] - e1 * e2).max() <= 1e-12


def test_contribution_rule_stops_a_ray():
    """Once 1 - T reaches the limit nothing is added and T stays: with limit 0.5 in a constant medium the ray ends with
    the opacity of the first sample count that reaches 0.5."""
    sigma, dt = 2.0, 0.125
    table = np.tile(np.array([1.0, 1.0, 1.0, sigma]), (2, 1))
    o, d = np.array([[-3.0, 0.0, 0.0]], np.float32), np.array([[1.0, 0.0, 0.0]], np.float32)
    st, _ = _march(o, d, RR.BOX, dt, table, -1.0, 1.0, lambda p: np.zeros(p.shape[0]), limit=0.5)
    m = math.ceil(math.log(2.0) / (sigma * dt))                    # first m with 1 - exp(-sigma m dt) >= 0.5
    assert abs((1 - st[0, 3]) - (1 - math.exp(-sigma * m * dt))) <= 1e-12 and m < 16


# ---- conditions the GPU tests rely on, checked here on the CPU -----------------------------------------------------------

def test_ray_set_covers_the_cases():
    o, d = RR.ray_set()
    assert o.shape == (544, 3) and o.dtype == np.float32
    zeros = (d[480:] == 0).sum(1)
    assert {1, 2, 3} <= set(zeros.tolist())
    for t_min, t_max in RR.clip_cases():
        tn, tf, n = RR.clip(o, d, RR.BOX[0], RR.BOX[1], t_min, t_max, RR.DT, RR.ray_max_steps())
        assert (n[:480] > 0).sum() > 100 and (n[:480] == 0).sum() > 50          # the image sees the box and its surroundings
        assert (n[480:] > 0).sum() >= 15 and (n[480:] == 0).sum() >= 15
        assert np.all(tf[n > 0] > tn[n > 0]) and np.all(tn[n == 0] == np.float32(t_min))
    tn, tf, n = RR.clip(o, d, RR.BOX[0], RR.BOX[1], 0.0, np.inf, RR.DT, RR.ray_max_steps())
    assert n.max() == RR.ray_max_steps()          # the ray without a direction inside the box: limited, not converted
    assert ((n > 32) & (n <= 64)).any() and ((n > 0) & (n < 32)).any() and (n > 64).any()


@pytest.mark.parametrize('shaded', [False, True])
@pytest.mark.parametrize('limit', [0.95, 1.0])
def test_composite_case_leaves_out_at_most_two_percent(limit, shaded):
    """The fixed seed keeps the float64 reference alone within the cap of rays left out for being decided within 1e-5 of
    the limit (the GPU test asserts the same cap on the same arrays)."""
    case = RR.composite_case(limit, shaded)
    out = RR.left_out(case['margin'], 1e-5)
    assert out.sum() <= 0.02 * out.size
    assert (case['n_steps'] > 64).any() and (case['n_steps'] < 32).any()
    if limit < 1.0:
        assert ((1 - case['ref'][:, 3]) >= limit).sum() >= 10      # the rule is exercised: rays that were stopped


# ---- rays ---------------------------------------------------------------------------------------------------------------

def test_pinhole_rays_geometry():
    eye, at, up = (2.3, 1.4, 1.7), (0.1, -0.05, 0.0), (0.0, 0.0, 1.0)
    W, H, fov = 9, 7, 38.0
    o, d = Render.pinhole_rays(eye, at, up, fov, W, H)
    assert o.shape == d.shape == (H * W, 3) and o.dtype == d.dtype == torch.float32 and not o.is_cuda
    assert np.allclose(d.double().norm(dim=1).numpy(), 1.0, rtol=0, atol=2e-7)
    assert torch.equal(o, torch.tensor(eye).expand(H * W, 3))
    # centre ray (odd image): through look_at
    c = d[(H // 2) * W + W // 2].double().numpy()
    to_at = np.array(at) - np.array(eye)
    assert np.allclose(c, to_at / np.linalg.norm(to_at), atol=2e-7)
    # field of view: the rays through the centres of the top and bottom pixel rows of the middle column make the angle of
    # an image plane (H - 1) / H as tall as the stated one
    top, bot = d[W // 2].double().numpy(), d[(H - 1) * W + W // 2].double().numpy()
    want = 2 * math.atan(math.tan(math.radians(fov) / 2) * (H - 1) / H)
    assert abs(math.acos(np.clip(top @ bot, -1, 1)) - want) <= 1e-6
    left, right = d[(H // 2) * W].double().numpy(), d[(H // 2) * W + W - 1].double().numpy()
    want_h = 2 * math.atan(math.tan(math.radians(fov) / 2) * (W / H) * (W - 1) / W)
    assert abs(math.acos(np.clip(left @ right, -1, 1)) - want_h) <= 1e-6
    # corner rays: the diagonal angle of that plane
    tl, br = d[0].double().numpy(), d[H * W - 1].double().numpy()
    hh, hw = math.tan(math.radians(fov) / 2) * (H - 1) / H, math.tan(math.radians(fov) / 2) * (W / H) * (W - 1) / W
    assert abs(math.acos(np.clip(tl @ br, -1, 1)) - 2 * math.atan(math.hypot(hh, hw))) <= 1e-6
    # row-major, row 0 on top (up = +z), x to the right: right = forward x up
    assert top[2] > bot[2]
    fwd = to_at / np.linalg.norm(to_at)
    rvec = np.cross(fwd, np.array(up))
    assert right @ rvec > 0 > left @ rvec
    img = d.view(H, W, 3)
    assert torch.all(img[:, 1:, :].double() @ torch.tensor(rvec) > img[:, :-1, :].double() @ torch.tensor(rvec))


def test_orthographic_rays_geometry():
    eye, at, up = (3.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)
    W, H = 5, 3
    o, d = Render.orthographic_rays(eye, at, up, 1.5, W, H)
    assert o.shape == d.shape == (H * W, 3)
    assert torch.equal(d, torch.tensor([-1.0, 0.0, 0.0]).expand(H * W, 3))
    assert torch.allclose(o[(H // 2) * W + W // 2], torch.tensor(eye))                    # centre ray through look_at
    assert abs(float(o[0, 2] - o[(H - 1) * W, 2]) - 1.5 * (H - 1) / H) <= 1e-6            # centres span (H-1)/H of the height
    assert abs(float((o[0] - o[W - 1]).norm()) - 1.5 * W / H * (W - 1) / W) <= 1e-6
    assert float(o[0, 2]) > float(o[(H - 1) * W, 2])                                      # row 0 on top


def test_ray_generators_refuse_degenerate_cameras():
    with pytest.raises(ValueError):
        Render.pinhole_rays((0, 0, 1), (0, 0, 1), (0, 0, 1), 40, 4, 4)
    with pytest.raises(ValueError):
        Render.pinhole_rays((0, 0, 1), (0, 0, 0), (0, 0, 1), 40, 4, 4)
    with pytest.raises(ValueError):
        Render.pinhole_rays((1, 0, 0), (0, 0, 0), (0, 0, 1), 180, 4, 4)
    with pytest.raises(ValueError):
        Render.orthographic_rays((1, 0, 0), (0, 0, 0), (0, 0, 1), 0.0, 4, 4)


# ---- transfer function --------------------------------------------------------------------------------------------------

def test_transfer_function_validation():
    good = [[0, 0, 0, 0], [1, 1, 1, 2.0]]
    tf = Render.TransferFunction(good)
    assert tf.table.shape == (2, 4) and tf.v_min == -1.0 and tf.v_max == 1.0
    with pytest.raises(ValueError):
        Render.TransferFunction([[0, 0, 0, 1.0]])                   # K < 2
    with pytest.raises(ValueError):
        Render.TransferFunction([[0, 0, 0], [1, 1, 1]])             # not (K, 4)
    with pytest.raises(ValueError):
        Render.TransferFunction([[0, 0, 0, 0], [1, 1, 1, -0.1]])    # negative extinction
    with pytest.raises(ValueError):
        Render.TransferFunction(good, v_min=0.5, v_max=0.5)         # v_max <= v_min
    with pytest.raises(ValueError):
        Render.TransferFunction(good, v_min=0.5, v_max=-0.5)
    with pytest.raises(ValueError):
        Render.TransferFunction([[0, 0, 0, 0], [1, 1, 1, float('nan')]])


# ---- no CPU form ----------------------------------------------------------------------------------------------------------

def test_cpu_tensors_raise():
    from latent_feature_grid_compression_amd import ops
    o, d = Render.pinhole_rays((3, 0, 0), (0, 0, 0), (0, 0, 1), 30, 4, 4)
    tf = Render.TransferFunction([[0, 0, 0, 0], [1, 1, 1, 2.0]])
    with pytest.raises(LfgcError):
        Render.render_from_net([1.0, 1.0, 1.0], torch.nn.Identity(), o, d, tf, step=0.1)
    with pytest.raises(LfgcError):
        Render.render(lambda p: p[:, 0], o, d, tf, 0.1, [-1, -1, -1], [1, 1, 1])
    with pytest.raises(LfgcError):
        ops.ray_clip(o, d, [-1, -1, -1], [1, 1, 1], 0.1, 100)
    i32 = torch.zeros(16, dtype=torch.int32)
    with pytest.raises(LfgcError):
        ops.ray_compact(None, i32, i32, torch.zeros(16, 4), 0.99)


def test_render_arguments_are_checked_before_any_launch():
    tf = Render.TransferFunction([[0, 0, 0, 0], [1, 1, 1, 2.0]])
    assert Render.max_steps_for([-1, -1, -1], [1, 1, 1], 0.01) == math.ceil(2 * math.sqrt(12) / 0.01)
    assert Render.image_psnr(torch.zeros(4, 4), torch.zeros(4, 4)) == float('inf')
    assert abs(Render.image_psnr(torch.zeros(4, 4), torch.full((4, 4), 0.1)) - 20.0) <= 1e-5
    img = torch.tensor([[0.2, 0.1, 0.0, 0.75]])
    assert torch.allclose(Render.background(img, (1.0, 1.0, 0.0)), torch.tensor([[0.45, 0.35, 0.0]]))
    assert tf.on('cpu') is tf.on('cpu')
