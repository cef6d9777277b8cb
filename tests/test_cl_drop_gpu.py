"""GPU tests of the channel-last last level with the pruning ("drop") layers folded in: ops.idwt_level_cl_drop /
ops.idwt_level_cl_drop_bwd (lfgc_idwt_level_cl_drop_len_f32 and its adjoint) and the decode nodes that route their last
level through them.

References: the oracle's autograd (R.wavelet_decode on the factor-applied coefficients, channel-first, permuted for the
comparison), the channel-first DROP level + layout conversion (tests/test_hip_drop.py pins that one to the reference), and
the plain channel-last level for the bitwise properties.  Tolerances are the project's for the same quantities
(test_idwt_level_with_factors_forward_backward, test_last_level_channel_last_kernels): decoded grids 1e-5 of the tensor
maximum, gradients -- sums accumulated in another order -- 2e-5 of the largest entry of the tensor."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_drop as D
from oracle import ref_torch as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def rel_err(y, ref):
    y = np.asarray(y, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    return np.abs(y - ref).max() / max(np.abs(ref).max(), 1e-30)


def filters(basis):
    """filter_rev fp32 CPU: db2 from the oracle's recipe, Haar as captured from the reference."""
    if basis == 'db2':
        return R.build_filters(3)[1]
    with np.load(os.path.join(GOLD, 'wavelets_filters.npz')) as z:
        return torch.from_numpy(z['filter_rev_2'])


CL_CASES = [   # copy of tests/test_hip_forward.py: (C, d, t): channel counts around every stride, ragged planes, every crop
    (1, (3, 4, 5), (7, 9, 11)), (5, (6, 7, 9), (13, 15, 19)), (8, (9, 9, 9), (16, 16, 16)), (13, (5, 12, 7), (10, 24, 14)),
    (16, (17, 17, 17), (32, 32, 32)), (22, (4, 35, 6), (9, 69, 13)), (24, (10, 11, 12), (19, 21, 23)),
    (30, (8, 9, 40), (17, 18, 81)), (32, (17, 18, 16), (33, 34, 31)), (32, (33, 33, 33), (64, 64, 64)),
    (3, (1, 1, 1), (2, 3, 4)), (32, (2, 70, 3), (5, 140, 6)),
    (40, (5, 6, 7), (11, 13, 15)),      # C > 32: the wrappers fall back to level + layout conversion
    # large planes: 16-wave synthesis workgroups (32 channels), 64-cell adjoint tiles (16- and 8-channel groups)
    (32, (2, 64, 64), (5, 129, 128)), (16, (2, 64, 64), (4, 128, 128)), (8, (3, 60, 60), (6, 119, 120)),
    (32, (65, 65, 65), (128, 128, 128)),   # cfg-5 last level: streaming stores (grid > 48 MiB)
]
# straight against the oracle: the ragged shapes (channel counts off every stride, non-cubic planes, every crop)
# (and, by name, the C = 40 case: there both sides of the comparison with the channel-first path are the same fallback
# composition, so the oracle is its only independent reference)
C40_CASE = (40, (5, 6, 7), (11, 13, 15))
assert C40_CASE in CL_CASES
ORACLE_CASES = [c for c in CL_CASES if c[0] * np.prod(c[2]) <= 300000 and c != C40_CASE] + [C40_CASE]
assert sum(1 for C, d, t in ORACLE_CASES if len(set(d)) > 1 or C % 8) >= 5


def level_target(basis, d, t):
    """The list's targets are db2's (up to 2 d + 2 per axis); a Haar level is at most 2 d wide."""
    return tuple(t) if basis == 'db2' else tuple(min(tv, 2 * dv) for tv, dv in zip(t, d))


def make_inputs(C, d, t, seed):
    rng = np.random.default_rng(seed)
    lll = torch.from_numpy(rng.standard_normal((C,) + tuple(d)).astype(np.float32))
    hf = torch.from_numpy(rng.standard_normal((C, 7) + tuple(d)).astype(np.float32))
    ml = torch.from_numpy(rng.uniform(0.05, 1.0, tuple(d)).astype(np.float32))
    mh = torch.from_numpy(rng.uniform(0.05, 1.0, (7,) + tuple(d)).astype(np.float32))
    cs = (C + 7) // 8 * 8
    g_cl = torch.from_numpy(rng.standard_normal(tuple(t) + (cs,)).astype(np.float32))
    return lll, hf, ml, mh, g_cl


def applied(x, m, thr):
    """A coefficient tensor through its drop layer, autograd-visible (oracle/ref_drop.py rules)."""
    if m is None:
        return x
    if thr is None:
        return x * m.unsqueeze(0)
    return (x * (m >= thr) - x * m).detach() + x * m


@pytest.mark.parametrize('thr', [None, 0.5])
@pytest.mark.parametrize('basis', ['haar', 'db2'])
@pytest.mark.parametrize('C,d,t', CL_CASES)
def test_against_channel_first_drop_path(dev, C, d, t, basis, thr):
    """The fused DROP last level against the channel-first DROP level + the layout conversion, with and without the
    low band's factor; pad channels exactly 0."""
    from latent_feature_grid_compression_amd import ops
    t = level_target(basis, d, t)
    frev = filters(basis).to(dev)
    lll, hf, ml, mh, g_cl = (x.to(dev) for x in make_inputs(C, d, t, C * 1000 + d[0] + (thr is not None)))
    cs = g_cl.shape[-1]
    for with_low in (True, False):
        m_l = ml if with_low else None
        want = ops.to_channel_last(ops.idwt_level_drop(lll, hf, m_l, thr, mh, thr, frev, t))
        got = ops.idwt_level_cl_drop(lll, hf, m_l, thr, mh, thr, frev, t)
        assert got.shape == want.shape == tuple(t) + (cs,)
        err = rel_err(got.cpu().numpy(), want.cpu().numpy())
        print('forward', basis, thr, with_low, err)
        assert err <= 1e-5
        if cs > C:
            assert np.array_equal(got[..., C:].cpu().numpy(), np.zeros(tuple(t) + (cs - C,), np.float32))
        w = ops.idwt_level_drop_bwd(ops.to_channel_first(g_cl, C), frev, lll, hf, m_l, mh, with_low, True, d)
        g = ops.idwt_level_cl_drop_bwd(g_cl, C, frev, lll, hf, m_l, mh, with_low, True, d)
        for name, a, b in zip(('d_lll', 'd_hf', 'd_mul_lll', 'd_mul_hf'), g, w):
            assert (a is None) == (b is None), name
            if a is not None:
                err = rel_err(a.cpu().numpy(), b.cpu().numpy())
                print(name, basis, thr, with_low, err)
                assert err <= 2e-5, name


@pytest.mark.parametrize('thr', [None, 0.5])
@pytest.mark.parametrize('basis', ['haar', 'db2'])
@pytest.mark.parametrize('C,d,t', ORACLE_CASES)
def test_against_oracle_autograd(dev, C, d, t, basis, thr):
    from latent_feature_grid_compression_amd import ops
    t = level_target(basis, d, t)
    frev = filters(basis)
    lll, hf, ml, mh, g_cl = make_inputs(C, d, t, C * 77 + d[1] + (thr is not None))
    cs = g_cl.shape[-1]
    for with_low in (True, False):
        leaves = [x.clone().requires_grad_(True) for x in (lll, hf, ml, mh)]
        a = applied(leaves[0], leaves[2] if with_low else None, thr)
        b = applied(leaves[1], leaves[3], thr)
        ref = R.wavelet_decode(torch.cat([a.unsqueeze(0).unsqueeze(2), b.unsqueeze(0)], dim=2), t, frev)[0]
        (ref * g_cl[..., :C].permute(3, 0, 1, 2)).sum().backward()
        m_l = ml.to(dev) if with_low else None
        got = ops.idwt_level_cl_drop(lll.to(dev), hf.to(dev), m_l, thr, mh.to(dev), thr, frev.to(dev), t)
        err = rel_err(got[..., :C].permute(3, 0, 1, 2).cpu().numpy(), ref.detach().numpy())
        print('forward', basis, thr, with_low, err)
        assert err <= 1e-5
        if cs > C:
            assert float(got[..., C:].abs().max()) == 0.0
        g = ops.idwt_level_cl_drop_bwd(g_cl.to(dev), C, frev.to(dev), lll.to(dev), hf.to(dev), m_l, mh.to(dev), with_low, True, d)
        wants = (leaves[0].grad, leaves[1].grad, leaves[2].grad if with_low else None, leaves[3].grad)
        for name, x, want in zip(('d_lll', 'd_hf', 'd_mul_lll', 'd_mul_hf'), g, wants):
            assert (x is None) == (want is None), name
            if x is not None:
                err = rel_err(x.cpu().numpy(), want.numpy())
                print(name, basis, thr, with_low, err)
                assert err <= 2e-5, name


@pytest.mark.parametrize('basis', ['haar', 'db2'])
@pytest.mark.parametrize('C,d,t', CL_CASES)
def test_bitwise_properties(dev, C, d, t, basis):
    """Forward: plain-product factors give exactly the plain channel-last level of the pre-multiplied coefficients (the
    same fp32 product, the same contraction), pad channels exactly 0.  Adjoint: all-ones factors and no penalties give
    exactly the plain adjoint; with every factor and penalty pointer NULL the entries ARE the plain ones."""
    from latent_feature_grid_compression_amd import ops, _lib
    t = level_target(basis, d, t)
    frev = filters(basis).to(dev)
    lll, hf, ml, mh, g_cl = (x.to(dev) for x in make_inputs(C, d, t, C * 31 + d[2]))
    cs = g_cl.shape[-1]
    for m_l in (ml, None):
        got = ops.idwt_level_cl_drop(lll, hf, m_l, None, mh, None, frev, t)
        pre_l = lll if m_l is None else lll * m_l.unsqueeze(0)
        want = ops.idwt_level_cl(pre_l, hf * mh.unsqueeze(0), frev, t)
        assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
        if cs > C:
            assert np.array_equal(got[..., C:].cpu().numpy(), np.zeros(tuple(t) + (cs - C,), np.float32))
    w_l, w_h = ops.idwt_level_cl_bwd(g_cl, C, frev, d)
    one_l, one_h = torch.ones_like(ml), torch.ones_like(mh)
    for m_l, want_l in ((one_l, True), (one_l, False), (None, False)):
        g_l, g_h, _, _ = ops.idwt_level_cl_drop_bwd(g_cl, C, frev, lll, hf, m_l, one_h, want_l, True, d)
        assert np.array_equal(g_l.cpu().numpy(), w_l.cpu().numpy())
        assert np.array_equal(g_h.cpu().numpy(), w_h.cpu().numpy())
    if C <= 32:             # the raw entries with every optional pointer NULL (C > 32 is refused: the wrappers fall back)
        lib = _lib.load()
        taps, L = ops.filter_taps(frev), ops.filter_length(frev)
        out = torch.empty(tuple(t) + (cs,), device=dev)
        nan = float('nan')
        assert lib.lfgc_idwt_level_cl_drop_len_f32(lll.data_ptr(), hf.data_ptr(), None, nan, None, nan, taps, L, out.data_ptr(),
                                                   C, cs, *d, *t, None) == 0
        assert np.array_equal(out.cpu().numpy(), ops.idwt_level_cl(lll, hf, frev, t).cpu().numpy())
        d_l, d_h = torch.empty_like(lll), torch.empty_like(hf)
        assert lib.lfgc_idwt_level_cl_drop_bwd_len_f32(g_cl.data_ptr(), taps, L, lll.data_ptr(), hf.data_ptr(), None, None,
                                                       d_l.data_ptr(), d_h.data_ptr(), None, None, None, C, cs, *d, *t, None) == 0
        assert np.array_equal(d_l.cpu().numpy(), w_l.cpu().numpy()) and np.array_equal(d_h.cpu().numpy(), w_h.cpu().numpy())


def _penalty_run(dev, frev, shape_array, thresholds, l1_flags, coeffs, factors, w_cl, weights):
    from latent_feature_grid_compression_amd import ops
    n = len(coeffs)
    cs_in = [c.to(dev).requires_grad_(True) for c in coeffs]
    fs_in = [None if f is None else f.to(dev).requires_grad_(True) for f in factors]
    grid, pen = ops.DecodeVolumePenaltyFn.apply(frev.to(dev), shape_array, True, thresholds, n, l1_flags, *cs_in, *fs_in)
    ((grid * w_cl.to(dev)).sum() + (pen * weights.to(dev)).sum()).backward()
    return grid.detach().cpu(), pen.detach().cpu(), [c.grad.cpu() for c in cs_in], [None if f is None else f.grad.cpu() for f in fs_in]


@pytest.mark.parametrize('basis', ['haar', 'db2'])
@pytest.mark.parametrize('levels', [1, 2])
def test_penalty_folds(dev, monkeypatch, basis, levels):
    """DecodeVolumePenaltyFn (L2 terms on every tensor, L1 flag on the factors) through the channel-last last level,
    against the same call under LFGC_CL_LEVEL=0 and against oracle autograd of grid . w + sum weights . penalties.
    C = 24 > 16: three channel groups in the adjoint -- the L1 term must be added once, not once per group.  One level:
    the last level is also the first (factors[0] is its low-band factor)."""
    C = 24
    frev = filters(basis)
    rng = np.random.default_rng(40 + levels)
    if levels == 1:
        dims, shape_array = [(6, 7, 5)], [(11, 13, 10)]
    else:
        dims, shape_array = [(4, 5, 4), (7, 9, 8)], [(7, 9, 8), (13, 17, 15)]
    coeffs = [torch.from_numpy(rng.standard_normal((C,) + dims[0]).astype(np.float32))]
    coeffs += [torch.from_numpy(rng.standard_normal((C, 7) + dd).astype(np.float32)) for dd in dims]
    factors = [torch.from_numpy((rng.uniform(0.05, 1.0, c.shape[1:]) * rng.choice([-1.0, 1.0], c.shape[1:])).astype(np.float32))
               for c in coeffs]                      # both signs: sign(m) matters
    n = len(coeffs)
    cs = 24
    w_cl = torch.zeros(tuple(shape_array[-1]) + (cs,))
    w_cl[..., :C] = torch.from_numpy(rng.standard_normal(tuple(shape_array[-1]) + (C,)).astype(np.float32))
    weights = torch.from_numpy(rng.uniform(0.5, 2.0, 2 * n).astype(np.float32))
    thresholds, l1_flags = [None] * n, [True] * n

    # the fused path must not convert layouts
    from latent_feature_grid_compression_amd import ops

    def refuse(*a, **k):
        raise AssertionError('layout conversion on the fused path')
    with monkeypatch.context() as mp:
        mp.setattr(ops, 'to_channel_last', refuse)
        mp.setattr(ops, 'to_channel_first', refuse)
        grid, pen, d_c, d_f = _penalty_run(dev, frev, shape_array, thresholds, l1_flags, coeffs, factors, w_cl, weights)
    monkeypatch.setenv('LFGC_CL_LEVEL', '0')
    grid0, pen0, d_c0, d_f0 = _penalty_run(dev, frev, shape_array, thresholds, l1_flags, coeffs, factors, w_cl, weights)
    monkeypatch.delenv('LFGC_CL_LEVEL')

    leaves_c = [c.clone().requires_grad_(True) for c in coeffs]
    leaves_f = [f.clone().requires_grad_(True) for f in factors]
    restored = leaves_c[0] * leaves_f[0].unsqueeze(0)
    for k in range(1, n):
        b = leaves_c[k] * leaves_f[k].unsqueeze(0)
        restored = R.wavelet_decode(torch.cat([restored.unsqueeze(0).unsqueeze(2), b.unsqueeze(0)], dim=2), shape_array[k - 1], frev)[0]
    pens = torch.stack([D.grid_l2_penalty([c]) for c in leaves_c] + [D.l1_penalty(f) for f in leaves_f])
    ((restored * w_cl[..., :C].permute(3, 0, 1, 2)).sum() + (pens * weights).sum()).backward()

    assert rel_err(grid[..., :C].permute(3, 0, 1, 2).numpy(), restored.detach().numpy()) <= 1e-5
    assert rel_err(grid.numpy(), grid0.numpy()) <= 1e-5
    assert rel_err(pen.numpy(), pens.detach().numpy()) <= 2e-6 and np.array_equal(pen.numpy(), pen0.numpy())
    for i in range(n):
        for name, got, old, want in (('coeff', d_c[i], d_c0[i], leaves_c[i].grad), ('factor', d_f[i], d_f0[i], leaves_f[i].grad)):
            e_old, e_ref = rel_err(got.numpy(), old.numpy()), rel_err(got.numpy(), want.numpy())
            print(name, i, basis, levels, e_old, e_ref)
            assert e_old <= 2e-5 and e_ref <= 2e-5, (name, i)
    # the L1 term alone, exactly once: the factor gradient minus the data term is weight * sign(m)
    for i in range(n):
        data_term = leaves_f[i].grad - weights[n + i] * torch.sign(factors[i])
        extra = (d_f[i] - data_term) / (weights[n + i] * torch.sign(factors[i]))
        assert float((extra - 1.0).abs().max()) <= 0.05, i       # 2 or 3 times would read 2.0 or 3.0


def _model(kind, wavelet, C, G, H, L, dev, seed):
    from latent_feature_grid_compression_amd.model.model_utils import setup_model
    from latent_feature_grid_compression_amd.model.Dropout_Layer import DropoutLayer
    DropoutLayer.set_threshold_list(None)
    torch.manual_seed(seed)
    return setup_model(3, H, 1, L, 'fourier', 2, kind, 0.025, 0.75, wavelet, C, G, '').to(dev).train()


def _train_step(m, kind, pos, seed):
    from latent_feature_grid_compression_amd.model.Smallify_Dropout import SmallifyLoss
    m.zero_grad(set_to_none=True)
    torch.manual_seed(seed)                      # the variational layer draws its noise from the device generator
    loss = m(pos).square().mean()
    if kind == 'smallify':
        loss = loss + SmallifyLoss(weight_l1=1e-3, weight_l2=1e-5)(m)
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('wavelet', ['db2', 'haar'])
@pytest.mark.parametrize('kind', ['smallify', 'masked_straight_through', 'variational'])
@pytest.mark.parametrize('C,G,H,L,n', [(5, 14, 32, 2, 4096), (32, 64, 128, 4, 32768)])    # a small ragged shape, cfg 3
def test_train_step_takes_no_layout_pass(dev, monkeypatch, kind, wavelet, C, G, H, L, n):
    """A train-mode forward + backward of a model with drop layers must complete with the layout conversions refused,
    and give the loss and every parameter gradient of the LFGC_CL_LEVEL=0 composition."""
    from latent_feature_grid_compression_amd import ops
    m = _model(kind, wavelet, C, G, H, L, dev, 5)
    assert len(m.feature_grid) >= 2
    torch.manual_seed(9)
    pos = torch.rand(n, 3, device=dev) * 2 - 1
    _train_step(m, kind, pos, 1)                 # first step: the losses announce that they consume the penalty sums

    def refuse(*a, **k):
        raise AssertionError('layout conversion on the fused path')
    with monkeypatch.context() as mp:
        mp.setattr(ops, 'to_channel_last', refuse)
        mp.setattr(ops, 'to_channel_first', refuse)
        loss, grads = _train_step(m, kind, pos, 2)
    monkeypatch.setenv('LFGC_CL_LEVEL', '0')
    loss0, grads0 = _train_step(m, kind, pos, 2)
    monkeypatch.delenv('LFGC_CL_LEVEL')
    print(kind, wavelet, C, 'loss', loss, loss0)
    assert abs(loss - loss0) <= 2e-5 * abs(loss0)
    assert set(grads) == set(grads0) and len(grads) >= len(list(m.feature_grid)) + 2
    for k in grads0:
        err = rel_err(grads[k], grads0[k])
        print(kind, wavelet, C, k, err)
        assert err <= 2e-5, k


@pytest.mark.parametrize('basis', ['haar', 'db2'])
def test_graph_capture_and_replay(dev, basis):
    """One decode + backward through the new path captured under torch.cuda.graph after an eager warm-up (single stream:
    no parallel branches), replayed twice on changed coefficient values, against eager."""
    from latent_feature_grid_compression_amd import ops
    C, dims, shape_array = 16, [(5, 6, 4), (9, 11, 8)], [(9, 11, 8), (17, 21, 15)]
    frev = filters(basis).to(dev)
    rng = np.random.default_rng(3)
    draw = lambda shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
    coeffs = [draw((C,) + dims[0])] + [draw((C, 7) + dd) for dd in dims]
    factors = [torch.from_numpy(rng.uniform(0.05, 1.0, tuple(c.shape[1:])).astype(np.float32)).to(dev) for c in coeffs]
    for x in coeffs + factors:
        x.requires_grad_(True)
    w = draw(tuple(shape_array[-1]) + (16,))
    params = coeffs + factors

    def step():
        for p in params:
            p.grad = None
        grid = ops.DecodeVolumeDropFn.apply(frev, shape_array, True, [None] * 3, 3, *coeffs, *factors)
        (grid * w).sum().backward()
        return grid.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                   # warm-up: one-time kernel attributes, allocator pools
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        grid_g = step()
    grads_g = [p.grad for p in params]
    for trial in range(2):
        with torch.no_grad():
            for c in coeffs:
                c.copy_(draw(tuple(c.shape)))
        graph.replay()
        torch.cuda.synchronize()
        got_grid = grid_g.cpu().numpy().copy()
        got = [g.cpu().numpy().copy() for g in grads_g]
        want_grid = step().cpu().numpy()         # eager, same values (p.grad is rebound: the graph's tensors stay intact)
        torch.cuda.synchronize()
        assert np.array_equal(got_grid, want_grid), trial
        for p, a in zip(params, got):
            assert rel_err(a, p.grad.cpu().numpy()) <= 2e-5, trial


def _strided(x):
    """The same values with the last two axes stored transposed (not contiguous)."""
    y = x.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not y.is_contiguous() and torch.equal(x, y)
    return y


@pytest.mark.parametrize('thr', [None, 0.5])
@pytest.mark.parametrize('channel_last', [False, True])
@pytest.mark.parametrize('basis', ['haar', 'db2'])
def test_decode_nodes_take_non_contiguous_inputs(dev, basis, channel_last, thr):
    """DecodeVolumeDropFn and DecodeVolumePenaltyFn on coefficient and factor tensors that are not contiguous against the
    same values stored contiguously: the kernels take raw addresses, so every level -- channel-first ones included --
    must lay its operands out itself.  Two levels; with channel_last level 1 is channel-first and level 2 channel-last.
    Grid, penalty sums (fixed-order fp64 reduction) and coefficient gradients (overwritten) are bit-equal; the factor
    gradients are float-atomic sums over the channels: 1e-6 of the largest entry, the bound of
    test_len_entries_bit_equal_plain_4tap for the same quantity.  The contiguous run against oracle autograd: 2e-5."""
    from latent_feature_grid_compression_amd import ops
    C, cs = 5, 8
    dims, targets = [(4, 5, 4), (7, 9, 8)], [(7, 9, 8), (13, 17, 15)]
    shape_array = [level_target(basis, dd, tt) for dd, tt in zip(dims, targets)]
    frev = filters(basis)
    rng = np.random.default_rng(17)
    coeffs = [torch.from_numpy(rng.standard_normal((C,) + dims[0]).astype(np.float32))]
    coeffs += [torch.from_numpy(rng.standard_normal((C, 7) + dd).astype(np.float32)) for dd in dims]
    factors = [torch.from_numpy((rng.uniform(0.05, 1.0, c.shape[1:]) * rng.choice([-1.0, 1.0], c.shape[1:])).astype(np.float32))
               for c in coeffs]
    n = len(coeffs)
    w_cf = torch.from_numpy(rng.standard_normal((C,) + tuple(shape_array[-1])).astype(np.float32))
    w = w_cf
    if channel_last:
        w = torch.zeros(tuple(shape_array[-1]) + (cs,))
        w[..., :C] = w_cf.permute(1, 2, 3, 0)
    weights = torch.from_numpy(rng.uniform(0.5, 2.0, 2 * n).astype(np.float32))
    thresholds = [thr] * n

    def run(penalty, layout):
        cs_in = [layout(c).to(dev).requires_grad_(True) for c in coeffs]
        fs_in = [layout(f).to(dev).requires_grad_(True) for f in factors]
        assert all(x.is_contiguous() == (layout is not _strided) for x in cs_in + fs_in)
        if penalty:
            grid, pen = ops.DecodeVolumePenaltyFn.apply(frev.to(dev), shape_array, channel_last, thresholds, n, [True] * n,
                                                        *cs_in, *fs_in)
            ((grid * w.to(dev)).sum() + (pen * weights.to(dev)).sum()).backward()
        else:
            grid, pen = ops.DecodeVolumeDropFn.apply(frev.to(dev), shape_array, channel_last, thresholds, n, *cs_in, *fs_in), None
            (grid * w.to(dev)).sum().backward()
        return (grid.detach().cpu(), None if pen is None else pen.detach().cpu(), [c.grad.cpu() for c in cs_in],
                [f.grad.cpu() for f in fs_in])

    leaves_c = [c.clone().requires_grad_(True) for c in coeffs]
    leaves_f = [f.clone().requires_grad_(True) for f in factors]
    restored = applied(leaves_c[0], leaves_f[0], thr)
    for k in range(1, n):
        b = applied(leaves_c[k], leaves_f[k], thr)
        restored = R.wavelet_decode(torch.cat([restored.unsqueeze(0).unsqueeze(2), b.unsqueeze(0)], dim=2), shape_array[k - 1], frev)[0]
    pens = torch.stack([D.grid_l2_penalty([c]) for c in leaves_c] + [D.l1_penalty(f) for f in leaves_f])
    data_loss = (restored * w_cf).sum()

    for penalty in (False, True):
        loss = data_loss + (pens * weights).sum() if penalty else data_loss
        want = torch.autograd.grad(loss, leaves_c + leaves_f, retain_graph=True)
        grid, pen, d_c, d_f = run(penalty, lambda x: x)
        grid_s, pen_s, d_c_s, d_f_s = run(penalty, _strided)
        assert torch.equal(grid, grid_s), penalty
        if penalty:
            assert torch.equal(pen, pen_s)
        for i in range(n):
            assert torch.equal(d_c[i], d_c_s[i]), (penalty, 'coeff', i)
            err = rel_err(d_f_s[i].numpy(), d_f[i].numpy())
            print('factor', i, basis, channel_last, thr, penalty, err)
            assert err <= 1e-6, (penalty, 'factor', i)
            e_c, e_f = rel_err(d_c[i].numpy(), want[i].numpy()), rel_err(d_f[i].numpy(), want[n + i].numpy())
            print('oracle', i, basis, channel_last, thr, penalty, e_c, e_f)
            assert e_c <= 2e-5 and e_f <= 2e-5, (penalty, i)
