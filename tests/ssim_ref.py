"""NumPy fp64 statement of the SSIM definition of DESIGN.md 3.4.1 / include/lfgc.h: a direct triple loop over the taps,
written from the formula.  ``ssim_map`` is the reference of the tests; ``ssim_map_separable`` evaluates the same moments
axis by axis and exists only to be compared with it."""
import numpy as np


def _setup(a, b, weights, strides):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and a.ndim == 3
    g = [np.asarray(w, dtype=np.float64).reshape(-1) for w in weights]
    s = [int(v) for v in strides]
    m = [(n - len(w)) // st + 1 for n, w, st in zip(a.shape, g, s)]
    assert all(v >= 1 for v in m) and all(v >= 1 for v in s)
    return a, b, g, s, m


def _ssim(mx, my, exx, eyy, exy, c1, c2, k):
    vx = k * (exx - mx * mx)
    vy = k * (eyy - my * my)
    vxy = k * (exy - mx * my)
    return ((2.0 * mx * my + c1) * (2.0 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def moments(a, b, weights, strides):
    """The five W-weighted moments of every window, each (m0, m1, m2): one pass per tap (t0, t1, t2) over all windows."""
    a, b, g, s, m = _setup(a, b, weights, strides)
    fields = (a, b, a * a, b * b, a * b)          # fp32 values held in fp64: the products are exact
    out = [np.zeros(m, dtype=np.float64) for _ in fields]
    for t0, g0 in enumerate(g[0]):
        for t1, g1 in enumerate(g[1]):
            for t2, g2 in enumerate(g[2]):
                W = g0 * g1 * g2
                sl = tuple(slice(t, t + (mm - 1) * st + 1, st) for t, mm, st in zip((t0, t1, t2), m, s))
                for acc, f in zip(out, fields):
                    acc += W * f[sl]
    return out


def ssim_map(a, b, weights, strides, c1, c2, cov_norm=1.0):
    """(map (m0, m1, m2), plane_sums (m0,)) in fp64."""
    with np.errstate(invalid='ignore'):
        smap = _ssim(*moments(a, b, weights, strides), c1, c2, cov_norm)
    return smap, smap.reshape(smap.shape[0], -1).sum(axis=1)


def ssim_map_separable(a, b, weights, strides, c1, c2, cov_norm=1.0):
    """The same moments, one axis after the other (axis 2 first)."""
    a, b, g, s, m = _setup(a, b, weights, strides)
    out = []
    for f in (a, b, a * a, b * b, a * b):
        for axis in (2, 1, 0):
            acc = 0.0
            for t, gt in enumerate(g[axis]):
                sl = [slice(None)] * 3
                sl[axis] = slice(t, t + (m[axis] - 1) * s[axis] + 1, s[axis])
                acc = acc + gt * f[tuple(sl)]
            f = acc
        out.append(f)
    smap = _ssim(*out, c1, c2, cov_norm)
    return smap, smap.reshape(smap.shape[0], -1).sum(axis=1)


def constants(data_range):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def covering_windows(index, shape, lengths, strides):
    """Boolean (m0, m1, m2): the windows that cover the element ``index``."""
    m = [(n - w) // st + 1 for n, w, st in zip(shape, lengths, strides)]
    axes = []
    for i, mm, w, st in zip(index, m, lengths, strides):
        o = np.arange(mm) * st
        axes.append((o <= i) & (i < o + w))
    return axes[0][:, None, None] & axes[1][None, :, None] & axes[2][None, None, :]


def make_field(shape, sigma, seed):
    """(a, b) fp32 in [-1, 1]: a smooth field with one flat half, b = a + sigma noise, every fourth x-plane of b equal to a."""
    rng = np.random.default_rng(seed)
    x, y, z = np.meshgrid(*[np.linspace(0.0, 1.0, n) if n > 1 else np.zeros(1) for n in shape], indexing='ij')
    a = np.sin(3.0 * x * 2.0 + 2.0 * y * 3.0) * np.cos(2.0 * z * 4.0)
    a[:, :, shape[2] // 2:] = 0.25                                  # the flat half
    a = np.clip(a, -1.0, 1.0).astype(np.float32)
    b = a + sigma * rng.standard_normal(shape).astype(np.float32)
    b[::4] = a[::4]
    return a, np.clip(b, -1.0, 1.0).astype(np.float32)
