"""GPU tests of the three routes a feature gradient takes into d_grid, and of the input-gradient build, on a grid whose
three extents differ.

All of them take the cell geometry from csrc/lfgc_trilinear.h: the data kernel's in-kernel scatter (default), the deferred
float scatter behind LFGC_SCATTER=deferred, the deterministic fixed-point scatter, and the INPUT_ONLY build whose
coordinate-gradient corner loop is the training build's.  A (6, 7, 9) grid shows a swapped axis; C = 5 / 16 / 22 / 32 are
channel strides 8 / 16 / 24 / 32, i.e. 8 / 4 / 2 / 2 samples per atomic wave-instruction (stride 24 leaves 16 lanes idle);
n = 77 is three 32-sample tiles, the last ragged.

Positions: those of tests/test_deterministic_gpu.py (the cube's corners, face centres, edge points, points out to +-2.2,
[1.2, -1.2, 0]) and, in the ragged tile, +1e10 and -1e10 on every axis (the unnormalised coordinate is past the int range:
the clamp to [-2, size] before the conversion is what keeps the cell defined) and -1 - 1/size on every axis (exactly one
cell below the first cell centre: floor() lands on -1).  Positions of +-1e30 or inf are left to the one-off comparison
of profiles/r8: there the device's wide trigonometric reduction (exact for |x| < 1e15, lfgc_common.h) returns non-finite
values, the sample's feature gradient is non-finite, and one such value turns the whole deterministic grid gradient NaN by
design, which would hide the comparison of the three routes.

Bounds (none derived from HIP output): d_grid against the oracle's autograd at 2e-5 of the largest entry, the bound of
tests/test_hip_backward.py for 'fp32' and 'f16x2'; d_pos of the input-gradient build at tests/test_gradient_gpu.py's TOL;
rows outside the grid, per component against the fp64 oracle, at max(3 x the fp32 oracle's own error, 2e-5) -- the d_pos
component rule of tests/test_kernel_matrix_gpu.py.  HIP against HIP is exact.

The two +-1e10 rows run through every route and every bitwise comparison, and must come out finite, but their d_pos is not
compared with an oracle: the position is itself a layer-0 input, so the pre-activations are about 1e9, and snake'(a) =
0.5 + sin(2a) of such a number depends on the last bits of a (one ulp is 64), i.e. on the order of the layer's sum.  The
fp32 and the fp64 oracle disagree with each other on these rows by the size of the gradient itself (asserted below: that
is why they are left out, and no other row may be)."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_forward import build_synth, rel_err, dev  # noqa: F401
from test_deterministic_gpu import _positions
from test_gradient_gpu import TOL

pytestmark = pytest.mark.gpu

SHAPE = (6, 7, 9)             # (D, H, W)
HID, LAYERS, N = 32, 2, 77
CHANNELS = [5, 16, 22, 32]
HUGE = 1e9                    # |p| from here on: the two rows described in the module docstring
_REF = {}


def route_positions():
    """(N, 3) fp32 positions of the module docstring."""
    p = _positions(N, 9).numpy().copy()
    D, H, W = SHAPE
    one = np.float32(1)
    p[N - 4] = [1e10, 1e10, 1e10]
    p[N - 3] = [-1e10, -1e10, -1e10]
    p[N - 2] = [-one - one / np.float32(W), -one - one / np.float32(H), -one - one / np.float32(D)]
    return torch.from_numpy(p)


def outside_rows(pos):
    """Rows with an axis on which both cells of the sample lie outside the grid (every corner weight is then zero): the
    kernels' own fp32 arithmetic, floor(((p + 1) size - 1) / 2) < -1 or >= size."""
    p = pos.numpy().astype(np.float32)
    size = np.asarray(SHAPE[::-1], np.float32)               # p[:, 0] runs along W
    f0 = np.floor(((p + np.float32(1)) * size - np.float32(1)) * np.float32(0.5))
    return ((f0 < -1) | (f0 >= size)).any(axis=1)


def upstream(n=N):
    return torch.from_numpy(np.random.default_rng(31).standard_normal(n).astype(np.float32))


def oracle_gradients(sm, pos, g, dtype):
    """d sum(g y) / d (dense grid, positions) by the oracle's autograd on the CPU -> ((D, H, W, C), (N, 3)) float64 numpy."""
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    to = lambda t: t.detach().to(dtype)                      # noqa: E731
    dense = R.decode_volume([to(c) for c in sm['coeffs']], sm['shape_array'], to(sm['filter_rev'])).requires_grad_(True)
    p = to(pos).clone().requires_grad_(True)
    y = R.forward_from_grid(dense, [to(w) for w in sm['weights']], [to(b) for b in sm['biases']], p, 2).squeeze(-1)
    (y * to(g)).sum().backward()
    return dense.grad.permute(1, 2, 3, 0).double().numpy(), p.grad.double().numpy()


def _case(C, dev_, g):
    """(model, synthetic parameters, positions, fp32 and fp64 oracle gradients for upstream gradient g), once per C."""
    key = (C, g is None)
    if key not in _REF:
        m, sm = build_synth(C, max(SHAPE), HID, LAYERS, seed=8100 + C, dev=dev_, grid_shape=SHAPE)
        m.train()
        pos = route_positions()
        gv = torch.ones(N) if g is None else g
        _REF.clear()
        _REF[key] = (m, sm, pos, oracle_gradients(sm, pos, gv, torch.float32), oracle_gradients(sm, pos, gv, torch.float64))
    return _REF[key]


def check_outside_rows(tag, d_pos, pos, dp32, dp64):
    """d_pos of the rows outside the grid: no sampler term, so what is left is the direct and the Fourier columns."""
    huge = (pos.abs() >= HUGE).any(dim=1).numpy()
    assert int(huge.sum()) == 2
    assert np.isfinite(d_pos).all() and np.isfinite(dp32).all() and np.isfinite(dp64).all()
    top = np.abs(dp64[~huge]).max()
    assert np.abs(dp32[huge] - dp64[huge]).max() > 1e-2 * top        # the oracle itself has no answer there
    rows = outside_rows(pos) & ~huge
    assert int(rows.sum()) >= 4
    ref = dp64[rows]
    scale = np.abs(ref).max(axis=0)
    e_hip = np.abs(d_pos[rows] - ref).max(axis=0) / scale
    e_cpu = float((np.abs(dp32[rows] - ref).max(axis=0) / scale).max())
    print('%s: outside rows %d, per component hip %s, fp32 oracle worst %.3e' % (tag, int(rows.sum()), e_hip, e_cpu))
    assert (e_hip <= max(3 * e_cpu, 2e-5)).all(), (tag, e_hip, e_cpu)
    return ~huge


@pytest.mark.parametrize('precision', ['fp32', 'f16x2'])
@pytest.mark.parametrize('C', CHANNELS)
def test_three_scatter_routes_agree_on_a_noncubic_grid(dev, C, precision, monkeypatch):
    from latent_feature_grid_compression_amd import ops
    g = upstream()
    m, sm, pos, (dg32, dp32), (_dg64, dp64) = _case(C, dev, g)
    desc = m._descriptor()
    with torch.no_grad():
        grid_cl, packed = m._decoded_channel_last(), m._packed()
    assert tuple(grid_cl.shape[:3]) == SHAPE
    weights, biases = m._mlp_params()
    pos_d, g_d = pos.to(dev), g.to(dev)
    _y, stash = ops.forward_raw(desc, grid_cl, packed, pos=pos_d, want_stash=True, precision=precision)

    def run(deterministic):
        out = ops.backward_raw(desc, grid_cl, packed, pos_d, stash, g_d, weights, biases, True, precision=precision,
                               deterministic=deterministic)
        torch.cuda.synchronize()
        return out

    monkeypatch.delenv('LFGC_SCATTER', raising=False)
    routes = {'in-kernel': run(False)}
    monkeypatch.setenv('LFGC_SCATTER', 'deferred')
    routes['deferred'] = run(False)
    monkeypatch.delenv('LFGC_SCATTER')
    routes['deterministic'] = run(True)

    assert np.isfinite(dg32).all() and np.abs(dg32).max() > 0
    for name, (d_grid, _dw, _db, _dp) in routes.items():
        got = d_grid[..., :C].cpu().numpy()
        e = rel_err(got, dg32)
        print('C%d %s %s: d_grid rel err %.3e' % (C, precision, name, e))
        assert np.isfinite(got).all() and e <= 2e-5, (name, e)
        assert int(torch.count_nonzero(d_grid[..., C:])) == 0, name          # the padding channels get nothing
    d_pos = routes['in-kernel'][3]
    for name in ('deferred', 'deterministic'):
        assert torch.equal(routes[name][3], d_pos), name                     # d_pos does not go through atomics
        for a, b in zip(routes[name][1] + routes[name][2], routes['in-kernel'][1] + routes['in-kernel'][2]):
            assert torch.equal(a, b), name                                   # nor do the weight gradients
    judged = check_outside_rows('C%d %s' % (C, precision), d_pos.cpu().double().numpy(), pos, dp32, dp64)
    assert rel_err(d_pos.cpu().numpy()[judged], dp32[judged]) <= 2e-5


@pytest.mark.parametrize('precision', ['fp32', 'f16x2'])
@pytest.mark.parametrize('C', CHANNELS)
def test_input_gradient_on_a_noncubic_grid(dev, C, precision):
    """lfgc_input_gradient_f32 (d_out = ones) on the same grid and positions against the oracle's d sum(y) / d pos."""
    from latent_feature_grid_compression_amd import ops
    m, _sm, pos, (_dg32, dp32), (_dg64, dp64) = _case(C, dev, None)
    desc = m._descriptor()
    with torch.no_grad():
        grid_cl, packed = m._decoded_channel_last(), m._packed()
    pos_d = pos.to(dev)
    _y, stash = ops.forward_raw(desc, grid_cl, packed, pos=pos_d, want_stash=True, precision=precision)
    got = ops.input_gradient_raw(desc, grid_cl, packed, pos_d, stash, precision=precision).cpu().double().numpy()
    judged = check_outside_rows('input gradient C%d %s' % (C, precision), got, pos, dp32, dp64)
    err = rel_err(got[judged], dp32[judged])
    print('input gradient C%d %s: rel err %.3e' % (C, precision, err))
    assert err <= TOL[precision]
