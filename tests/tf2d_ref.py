"""NumPy restatement of the 2-D transfer function's contract (include/lfgc.h: lfgc_ray_composite2d_f32,
lfgc_joint_histogram_f32) -- a helper, not a test.  Written from the contract, not from the kernels.

* ``composite2d`` in float64, one sample after the other, with the structure of render_ref.composite: its inputs are the
  float32 numbers the kernel gets, everything after that is float64.  The table is (Kv, Kg, 4) over
  [v_min, v_max] x [0, g_max]; the lookup interpolates along the value in both g rows, then along g.
* ``histogram_bins`` / ``histogram`` in float32, operation for operation as the contract states them (every float32
  operation of NumPy is correctly rounded and nothing is contracted), so the device counts are expected to be EQUAL.
* ``composite_case2d``: the shared inputs of the host and GPU tests."""
import numpy as np

import render_ref as RR

F = np.float32
G_MAX = 2.0


def lookup2d(table, v, gn, v_min, v_max, g_max):
    """float64 rgba (n, 4) of values v (n,) and gradient magnitudes gn (n,) in table (Kv, Kg, 4); a NaN takes row 0."""
    table = np.asarray(table, np.float64)
    Kv, Kg = table.shape[:2]
    with np.errstate(all='ignore'):
        u = np.fmin(np.fmax((np.asarray(v, np.float64) - v_min) * ((Kv - 1) / (float(v_max) - float(v_min))), 0.0), Kv - 1)
        w = np.fmin(np.fmax(np.asarray(gn, np.float64) * ((Kg - 1) / float(g_max)), 0.0), Kg - 1)
    i = np.minimum(u.astype(np.int64), Kv - 2)
    j = np.minimum(w.astype(np.int64), Kg - 2)
    f, h = (u - i)[:, None], (w - j)[:, None]
    lo = table[i, j] + f * (table[i + 1, j] - table[i, j])
    hi = table[i, j + 1] + f * (table[i + 1, j + 1] - table[i, j + 1])
    return lo + h * (hi - lo)


def composite2d(values, grads, dirs, tn, tf, n_steps, dt, table, v_min, v_max, g_max, limit, shaded, ka=0.3, kd=0.7, k_begin=0,
                state=None):
    """float64, sequential, as render_ref.composite with the 2-D lookup: grads (R, M, 3) are required, ``shaded`` adds the
    headlight.  Returns (state after, margin (R,))."""
    values = np.asarray(values, np.float64)
    grads = np.asarray(grads, np.float64)
    R, M = values.shape
    st = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (R, 1)) if state is None else np.array(state, np.float64)
    rgb, T = st[:, :3].copy(), st[:, 3].copy()
    margin = np.full(R, np.inf)
    d64 = np.asarray(dirs, np.float64)
    tn64, tf64, dt64 = np.asarray(tn, np.float64), np.asarray(tf, np.float64), float(F(dt))
    for m in range(M):
        k = np.full(R, k_begin + m, np.int64)
        valid = k < n_steps
        a = tn64 + k * dt64
        length = np.where(valid, np.maximum(np.minimum(a + dt64, tf64) - a, 0.0), 0.0)
        g = grads[:, m]
        gn = np.sqrt((g * g).sum(1))
        rgba = lookup2d(table, values[:, m], gn, v_min, v_max, g_max)
        alpha = 1.0 - np.exp(-rgba[:, 3] * length)
        shade = np.ones(R)
        if shaded:
            with np.errstate(all='ignore'):
                shade = np.where(gn > 0, ka + kd * np.abs((g * d64).sum(1)) / np.where(gn > 0, gn, 1.0), ka + kd)
        opacity = 1.0 - T
        margin = np.where(valid, np.minimum(margin, np.abs(opacity - limit)), margin)
        use = valid & (opacity < limit)
        rgb += np.where(use, T * alpha * shade, 0.0)[:, None] * rgba[:, :3]
        T = np.where(use, T * (1.0 - alpha), T)
    return np.concatenate([rgb, T[:, None]], 1), margin


def grad_norm_f32(grad):
    """sqrtf((gx*gx + gy*gy) + gz*gz) in float32."""
    g = np.asarray(grad, F)
    with np.errstate(all='ignore'):
        s = ((g[:, 0] * g[:, 0]).astype(F) + (g[:, 1] * g[:, 1]).astype(F)).astype(F)
        return np.sqrt((s + (g[:, 2] * g[:, 2]).astype(F)).astype(F)).astype(F)


def histogram_coordinates(values, grad, bins, v_min, v_max, g_max):
    """(u, w) float32: the table coordinates of a (Bv + 1, Bg + 1) table, with the float scales ops.joint_histogram passes."""
    Bv, Bg = bins
    v_scale, g_scale = F(Bv / (float(v_max) - float(v_min))), F(Bg / float(g_max))
    with np.errstate(all='ignore'):
        u = np.fmin(np.fmax(((np.asarray(values, F) - F(v_min)).astype(F) * v_scale).astype(F), F(0)), F(Bv)).astype(F)
        w = np.fmin(np.fmax(((grad_norm_f32(grad) - F(0)).astype(F) * g_scale).astype(F), F(0)), F(Bg)).astype(F)
    return u, w


def histogram_bins(values, grad, bins, v_min, v_max, g_max):
    """(i, j) int64 of every sample: i = min((int)u, Bv - 1), j = min((int)w, Bg - 1)."""
    u, w = histogram_coordinates(values, grad, bins, v_min, v_max, g_max)
    return np.minimum(u.astype(np.int64), bins[0] - 1), np.minimum(w.astype(np.int64), bins[1] - 1)


def histogram(values, grad, bins, v_min, v_max, g_max):
    i, j = histogram_bins(values, grad, bins, v_min, v_max, g_max)
    return np.bincount(i * bins[1] + j, minlength=bins[0] * bins[1]).reshape(bins).astype(np.int64)


def near_an_edge(values, grad, bins, v_min, v_max, g_max, ulps=4):
    """Samples whose restated coordinate lies within ``ulps`` float32 ulp of a bin edge (an integer) on either axis."""
    near = np.zeros(len(values), bool)
    for c in histogram_coordinates(values, grad, bins, v_min, v_max, g_max):
        edge = np.rint(c)
        near |= np.abs(c.astype(np.float64) - edge) <= ulps * np.spacing(np.maximum(edge, 1).astype(F)).astype(np.float64)
    return near


_CASES = {}


def composite_case2d(limit, shaded, seed=RR.COMPOSITE_SEED):
    """render_ref.composite_case(limit, True, seed)'s rays, values and gradients (present even when unshaded) under a random
    (7, 5, 4) table with rgb <= 1 and extinction <= 6 and g_max = 2: about 24 % of the samples clamp above g_max and 10 %
    have a gradient that is exactly zero.  A dict like composite_case's + the float64 reference and its margins."""
    key = (limit, bool(shaded), seed)
    if key not in _CASES:
        case = dict(RR.composite_case(limit, True, seed))
        rng = np.random.default_rng(seed + 100)
        table = np.concatenate([rng.uniform(0, 1, (7, 5, 3)), rng.uniform(0, 6, (7, 5, 1))], 2).astype(F)
        ref, margin = composite2d(case['values'], case['grads'], case['dirs'], case['t_near'], case['t_far'], case['n_steps'],
                                  RR.DT, table, -1.0, 1.0, G_MAX, limit, shaded)
        case.update(table=table, g_max=G_MAX, shaded=bool(shaded), ref=ref, margin=margin)
        _CASES[key] = case
    return _CASES[key]
