"""NumPy restatement of pre-integrated classification (include/lfgc.h: lfgc_ray_composite_preint_f32) --
a helper, not a test.  Written from the contract, not from the kernel.

Parameterised by dtype: float64 is the reference (its inputs are the float32 numbers the kernel gets, everything after
that is float64, as in render_ref.composite); float32, operation for operation in the order the contract states, only
sizes the tolerance of the GPU tests (``tolerance_factor``).  The integral table is float64 in both.  Also the shared
inputs of the host and GPU tests, each built once."""
import functools

import numpy as np

import render_ref as RR

F = np.float32


def integral(table):
    """pre (K, 4) float64: pre[0] = 0, pre[i] = the sum over c < i of B(c; 0, 1), row after row."""
    t = np.asarray(table, np.float64)
    pre = np.zeros_like(t)
    for c in range(t.shape[0] - 1):
        pre[c + 1] = pre[c] + bracket(t[c:c + 1], t[c + 1:c + 2], np.zeros(1), np.ones(1), np.float64)[0]
    return pre


def bracket(t0, t1, x0, x1, D=np.float64):
    """B(c; x0, x1) (n, 4) of the cells between the rows t0 and t1 (n, 4): the mean over [x0, x1] of (tau rgb, tau)."""
    t0, t1, x0, x1 = (np.asarray(a, D) for a in (t0, t1, x0, x1))
    d = t1 - t0
    s = (x0 + x1)[:, None]
    q3 = (((x0 * x0 + x0 * x1) + x1 * x1) / D(3))[:, None]
    w0, dw = t0[:, 3:4], d[:, 3:4]
    rgb = (w0 * t0[:, :3] + (D(0.5) * (w0 * d[:, :3] + dw * t0[:, :3])) * s) + (dw * d[:, :3]) * q3
    w = w0 + (D(0.5) * dw) * s
    return np.concatenate([rgb, w], 1).astype(D)


def cell(u, K, D=np.float64):
    i = np.minimum(np.asarray(u, D).astype(np.int64), K - 2)
    return i, (u - i.astype(D)).astype(D)


def slab_mean(table, pre, u_a, u_b, D=np.float64):
    """(c_bar (n, 3), tau_bar (n,), same (n,) bool) of the slabs between the table coordinates u_a and u_b."""
    tab = np.asarray(table, D)
    K = tab.shape[0]
    u_a, u_b = np.asarray(u_a, D), np.asarray(u_b, D)
    i_lo, f_lo = cell(np.fmin(u_a, u_b), K, D)
    i_hi, f_hi = cell(np.fmax(u_a, u_b), K, D)
    same = i_lo == i_hi
    one, zero = np.ones_like(f_lo), np.zeros_like(f_lo)
    m_same = bracket(tab[i_lo], tab[i_lo + 1], f_lo, np.where(same, f_hi, one), D)
    w_lo = (one - f_lo).astype(D)
    lo = bracket(tab[i_lo], tab[i_lo + 1], f_lo, one, D)
    hi = bracket(tab[i_hi], tab[i_hi + 1], zero, f_hi, D)
    mid = (np.asarray(pre, np.float64)[i_hi] - np.asarray(pre, np.float64)[np.minimum(i_lo + 1, K - 1)]).astype(D)
    m_diff = ((w_lo[:, None] * lo + mid) + f_hi[:, None] * hi).astype(D)
    length = ((w_lo + (i_hi - i_lo - 1).astype(D)) + f_hi).astype(D)
    m = np.where(same[:, None], m_same, m_diff).astype(D)
    with np.errstate(all='ignore'):
        tau = np.where(same, m[:, 3], m[:, 3] / np.where(same, one, length)).astype(D)
        lit = m[:, 3] > 0
        c_bar = np.where(lit[:, None], m[:, :3] / np.where(lit, m[:, 3], one)[:, None], D(0)).astype(D)
    return c_bar, tau, same


def coordinate(v, K, v_min, v_max, D=np.float64):
    """u(v): RR.tf_coordinate in float32; the same expression in float64 (a NaN lands in row 0)."""
    if D is F:
        return RR.tf_coordinate(v, K, v_min, v_max)
    tf_scale = (K - 1) / (float(v_max) - float(v_min))
    with np.errstate(all='ignore'):
        return np.fmin(np.fmax((np.asarray(v, np.float64) - v_min) * tf_scale, 0.0), float(K - 1))


def geometry(tn, tf, k, dt, D=np.float64):
    """(a, t_m, b) of segment k: float32 as lfgc_ray_samples_f32 forms them, or the same expressions in float64."""
    tn, tf, dt = np.asarray(tn, D), np.asarray(tf, D), D(F(dt))
    a = (tn + np.asarray(k).astype(D) * dt).astype(D)
    b = np.fmin((a + dt).astype(D), tf).astype(D)
    return a, (D(0.5) * (a + b).astype(D)).astype(D), b


def composite_preint(values, grads, dirs, tn, tf, n_steps, dt, table, v_min, v_max, limit, ka=0.3, kd=0.7, evaluated=None,
                     dtype=np.float64):
    """Sequential.  values (R, M): column m is sample k = m of every ray (columns with k >= n_steps are ignored); grads
    (R, M, 3) or None; ``evaluated`` (R, M) bool marks the samples that were composited (default: all) -- a sample whose
    predecessor was not opens with a half slab, which is what a jump of the skip kernel leaves behind.
    Returns (state (R, 4) = premultiplied r, g, b and T, margin (R,)) as render_ref.composite does."""
    D = dtype
    values = np.asarray(values)
    R, M = values.shape
    K = np.asarray(table).shape[0]
    pre = integral(table)
    ev = np.ones((R, M), bool) if evaluated is None else np.asarray(evaluated, bool)
    rgb, T = np.zeros((R, 3), D), np.ones(R, D)
    margin = np.full(R, np.inf)
    d = np.asarray(dirs, D)
    n_steps = np.asarray(n_steps)
    one = np.ones(R, D)
    for m in range(M):
        k = np.full(R, m, np.int64)
        valid = (k < n_steps) & ev[:, m]
        joined = valid & (ev[:, m - 1] if m > 0 else np.zeros(R, bool))
        a, tm, b = geometry(tn, tf, k, dt, D)
        _, tm_prev, _ = geometry(tn, tf, np.maximum(k - 1, 0), dt, D)
        length = np.fmax((tm - np.where(joined, tm_prev, a)).astype(D), D(0))
        close = np.fmax((b - tm).astype(D), D(0))
        u = coordinate(values[:, m], K, v_min, v_max, D)
        u_prev = coordinate(values[:, m - 1], K, v_min, v_max, D) if m > 0 else u
        c1, tau1, _ = slab_mean(table, pre, np.where(joined, u_prev, u), u, D)
        c2, tau2, _ = slab_mean(table, pre, u, u, D)
        a1 = (one - np.exp((-tau1 * length).astype(D))).astype(D)
        a2 = (one - np.exp((-tau2 * close).astype(D))).astype(D)
        shade = one
        if grads is not None:
            g = np.asarray(grads[:, m], D)
            gn = np.sqrt(((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(D)).astype(D)
            dot = np.abs(((g[:, 0] * d[:, 0] + g[:, 1] * d[:, 1]) + g[:, 2] * d[:, 2]).astype(D))
            with np.errstate(all='ignore'):
                shade = np.where(gn > 0, D(ka) + (D(kd) * dot) / np.where(gn > 0, gn, one), D(ka) + D(kd)).astype(D)
        last = k == n_steps - 1
        e = ((a1 * shade)[:, None] * c1).astype(D)
        e = np.where(last[:, None], e + ((((one - a1) * a2) * shade)[:, None] * c2), e).astype(D)
        factor = np.where(last, (one - a1) * (one - a2), one - a1).astype(D)
        opacity = (one - T).astype(D)
        margin = np.where(valid, np.minimum(margin, np.abs(opacity.astype(np.float64) - limit)), margin)
        use = valid & (opacity < D(limit))
        rgb = (rgb + np.where(use[:, None], T[:, None] * e, D(0))).astype(D)
        T = np.where(use, T * factor, T).astype(D)
    return np.concatenate([rgb, T[:, None]], 1), margin


def tolerance_factor(case, dt=RR.DT, ka=0.3, kd=0.7):
    """(k, ratio): ratio = max |float32 restatement - float64 restatement| / render_ref.composite_bound(n) over the rays of
    ``case`` that are not left out; the GPU bound is k * composite_bound with k = 2 * max(1, ratio).  ``case``: values,
    grads, dirs, t_near, t_far, n_steps, table, v_min, v_max, limit, evaluated (or None), steps, and the float64 ref and
    margin."""
    args = (case['values'], case['grads'], case['dirs'], case['t_near'], case['t_far'], case['n_steps'], dt, case['table'],
            case['v_min'], case['v_max'], case['limit'], ka, kd)
    low, _ = composite_preint(*args, evaluated=case['evaluated'], dtype=F)
    keep = ~RR.left_out(case['margin'], 1e-5)
    bound = RR.composite_bound(case['steps'])[:, None]
    ratio = float((np.abs(low.astype(np.float64) - case['ref']) / bound)[keep].max())
    return 2.0 * max(1.0, ratio), ratio


# ---- shared inputs ------------------------------------------------------------------------------------------------------

JUMP_EVERY = 3          # the jump case: rays 0, 3, 6, ... jump between the first and the second call, rays 1, 4, 7, ... before the first


@functools.lru_cache(maxsize=None)
def preint_case(limit, shaded, walk=False, jumps=False):
    """render_ref.composite_case(limit, shaded) -- 100 rays, three blocks of S = 32, its values, gradients, rays and K = 7
    table -- with the float64 pre-integrated reference.  ``walk``: the values are a slow random walk instead, so that
    neighbouring samples mostly share a table cell.  ``jumps``: as the skip kernel would move them, rays 0, 3, 6, ... jump
    over samples 32..63 between the first and the second call and rays 1, 4, 7, ... over samples 0..31 before the first
    ('evaluated' marks what three calls then composite; a fourth block of values and gradients is appended for them)."""
    base = RR.composite_case(limit, shaded)
    S, blocks = base['S'], base['blocks']
    values, grads = base['values'], base['grads']
    if walk:
        rng = np.random.default_rng(77)
        values = (rng.uniform(-1.1, 1.1, (100, 1)) + np.cumsum(rng.normal(0.0, 0.01, values.shape), 1)).astype(F)
    evaluated = np.ones(values.shape, bool)
    if jumps:
        rng = np.random.default_rng(78)
        values = np.concatenate([values, rng.uniform(-1.2, 1.2, (100, S)).astype(F)], 1)
        if shaded:
            grads = np.concatenate([grads, rng.normal(size=(100, S, 3)).astype(F)], 1)
        evaluated = np.ones(values.shape, bool)
        evaluated[0::JUMP_EVERY, S:2 * S] = False
        evaluated[1::JUMP_EVERY, :S] = False
        evaluated[2::JUMP_EVERY, blocks * S:] = False
    ref, margin = composite_preint(values, grads, base['dirs'], base['t_near'], base['t_far'], base['n_steps'], RR.DT,
                                   base['table'], -1.0, 1.0, limit, evaluated=evaluated)
    steps = np.minimum(base['n_steps'], blocks * S)               # what composite_bound takes, with or without jumps
    case = dict(base, values=values, grads=grads, evaluated=evaluated, ref=ref, margin=margin, steps=steps, v_min=-1.0, v_max=1.0)
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def ramp_case(step, n_rays=4):
    """The linear ramp of the issue: a K = 33 table over [-1, 1], transparent except for a spike of extinction 40 at row 16
    (rows 15..17 = 0, 40, 0), constant colour; v runs linearly from -0.9 at t_near = 1 to 0.9 at t_far = 2.7.  ``n_rays``
    identical rays.  Returns the inputs, the float64 values at the float64 t_m(k) ('values'; 'values32' is what a device
    gets) and the closed-form opacity 1 - exp(-(integral of tau dv) / |dv/dt|) = 0.905685."""
    table = np.zeros((33, 4), F)
    table[:, :3] = (0.2, 0.5, 0.8)
    table[16, 3] = 40.0
    tn, tf = np.full(n_rays, 1.0, F), np.full(n_rays, 2.7, F)
    n = np.full(n_rays, int(np.ceil((tf[0] - tn[0]) / F(step))), np.int32)
    M = 32 * ((int(n[0]) + 31) // 32)
    k = np.minimum(np.tile(np.arange(M), (n_rays, 1)), n[:, None] - 1)
    slope = 1.8 / (np.float64(tf[0]) - np.float64(tn[0]))      # dv/dt
    _, tm, _ = geometry(tn[:, None], tf[:, None], k, step)
    values = -0.9 + slope * (tm - 1.0)
    values32 = (-0.9 + slope * (RR.t_mid(tn[:, None], tf[:, None], k, step).astype(np.float64) - 1.0)).astype(F)
    area = 40.0 * (2.0 / 32.0)                                 # the integral of tau dv: a triangle two cells wide
    dirs = np.tile(np.array([[1.0, 0.0, 0.0]], F), (n_rays, 1))
    return dict(table=table, t_near=tn, t_far=tf, n_steps=n, values=values, values32=values32, dirs=dirs, step=step, M=M,
                colour=table[0, :3].astype(np.float64), opacity=1.0 - np.exp(-area / slope))
