"""GPU tests of the deterministic mode (model.deterministic / torch.use_deterministic_algorithms): the grid gradient is
scattered in 64-bit fixed point with integer atomics (order-independent), the drop factors' gradients get one writer per
address and a fixed-order fold.  Bitwise claims are checked with torch.equal; accuracy against the oracle's autograd at the
bound of tests/test_hip_backward.py, 2e-5 of each tensor's largest entry (each contribution is rounded once, by at most
2^-(61 - ceil(log2(8 n))) of the largest feature gradient: far below fp32's own rounding)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_forward import build_synth, rel_err, dev  # noqa: F401

pytestmark = pytest.mark.gpu

SMALL = [(5, 4, 4, 2, 3000),       # 4^3 grid (no wavelet level), ~370 contributions per cell, CH = 8
         (24, 7, 20, 3, 1000),     # CH = 24: idle lanes in the scatter
         (32, 8, 32, 2, 1000),     # CH = 32
         (3, 15, 100, 1, 77)]      # less than one tile


def _positions(n, seed):
    """n positions: the cube's corners, face centres and edge points, points up to 1.2 outside the cube, the rest inside."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    special = [[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    special += [[s if a == k else 0.25 for a in range(3)] for k in range(3) for s in (-1, 1)]        # faces
    special += [[-1, 1, 0.3], [1, 0.5, -1], [0.0, 0.0, 0.0]]
    outside = rng.uniform(-2.2, 2.2, (max(4, n // 10), 3)).astype(np.float32)
    outside[0] = [1.2, -1.2, 0.0]
    outside[1] = [2.2, 2.2, 2.2]
    rows = np.concatenate([np.asarray(special, np.float32), outside])[:n // 2]
    p[:len(rows)] = rows
    return torch.from_numpy(p)


def _raw_backward(m, pos, g, deterministic, precision='fp32'):
    from latent_feature_grid_compression_amd import ops
    desc = m._descriptor()
    with torch.no_grad():
        grid_cl = m._decoded_channel_last()
        packed = m._packed()
    weights, biases = m._mlp_params()
    y, stash = ops.forward_raw(desc, grid_cl, packed, pos=pos, want_stash=True, precision=precision)
    out = ops.backward_raw(desc, grid_cl, packed, pos, stash, g, weights, biases, True, precision=precision,
                           deterministic=deterministic)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('C,G,H,L,n', SMALL)
def test_grid_gradient_is_independent_of_the_sample_order(dev, C, G, H, L, n):
    m, _ = build_synth(C, G, H, L, seed=100 + C, dev=dev)
    m.train()
    pos = _positions(n, C).to(dev)
    g = torch.from_numpy(np.random.default_rng(G).standard_normal(n).astype(np.float32)).to(dev)
    d_grid, d_w, d_b, d_pos = _raw_backward(m, pos, g, True)
    assert bool(torch.isfinite(d_grid).all()) and float(d_grid.abs().max()) > 0
    for seed in (1, 2):
        perm = torch.from_numpy(np.random.default_rng(seed).permutation(n)).to(dev)
        d_grid_p, _, _, d_pos_p = _raw_backward(m, pos[perm].contiguous(), g[perm].contiguous(), True)
        assert torch.equal(d_grid, d_grid_p)
        assert torch.equal(d_pos[perm], d_pos_p)
    # and it is the default mode's gradient (float atomics) to rounding
    d_grid_0 = _raw_backward(m, pos, g, False)[0]
    assert rel_err(d_grid.cpu().numpy(), d_grid_0.cpu().numpy()) <= 1e-5


@pytest.mark.parametrize('precision', ['f16x2', 'fp32', 'f16'])
def test_gradients_are_bitwise_repeatable_and_follow_the_torch_switch(dev, precision, monkeypatch):
    from latent_feature_grid_compression_amd import ops
    m, _ = build_synth(16, 16, 32, 2, seed=77, dev=dev)
    m.train()
    m.precision = precision
    pos = torch.rand(3000, 3, device=dev) * 2 - 1
    seen = []
    real = ops.backward_raw

    def spy(*a, **k):
        seen.append(k.get('deterministic'))
        return real(*a, **k)
    monkeypatch.setattr(ops, 'backward_raw', spy)

    def run():
        m.zero_grad(set_to_none=True)
        m(pos.clone().requires_grad_(True)).square().mean().backward()
        return {k: p.grad.clone() for k, p in m.named_parameters()}

    m.deterministic = True
    outs = [run() for _ in range(3)]
    assert seen == [True] * 3
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[1][k], outs[2][k]), k
    assert any(k.startswith('feature_grid') for k in outs[0])
    # None follows torch's switch; True / False override it
    m.deterministic = None
    before = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        assert ops.deterministic_enabled()
        del seen[:]
        follow = run()
        m.deterministic = False
        run()
        assert seen == [True, False]
        m.deterministic = None
        torch.use_deterministic_algorithms(False)
        assert not ops.deterministic_enabled()
        del seen[:]
        run()
        assert seen == [False]
    finally:
        torch.use_deterministic_algorithms(before)
    for k in outs[0]:
        assert torch.equal(outs[0][k], follow[k]), k


def _oracle_grads(sm, L, pos, loss_of):
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    coeffs = [c.clone().requires_grad_(True) for c in sm['coeffs']]
    ws = [w.clone().requires_grad_(True) for w in sm['weights']]
    bs = [b.clone().requires_grad_(True) for b in sm['biases']]
    pos_r = pos.clone().requires_grad_(True)
    yr = R.forward(coeffs, sm['shape_array'], sm['filter_rev'], ws, bs, pos_r, 2, training=True)
    lr = loss_of(yr.squeeze(-1), lambda t: t)
    lr.backward()
    ref = {'feature_grid.%d' % i: c.grad.numpy() for i, c in enumerate(coeffs)}
    for i in range(L):
        ref['net_layers.%d.weight' % i], ref['net_layers.%d.bias' % i] = ws[i].grad.numpy(), bs[i].grad.numpy()
    ref['final_layer.weight'], ref['final_layer.bias'] = ws[L].grad.numpy(), bs[L].grad.numpy()
    return lr.item(), ref, pos_r.grad.numpy()


def _parity(dev, C, G, H, L, precision, pos, loss_of):
    m, sm = build_synth(C, G, H, L, seed=5000 + C + G + H, dev=dev)
    m.train()
    m.precision = precision
    m.deterministic = True
    pos_d = pos.to(dev).requires_grad_(True)
    loss = loss_of(m(pos_d).squeeze(-1), lambda t: t.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    loss_ref, ref, pos_ref = _oracle_grads(sm, L, pos, loss_of)
    assert abs(loss.item() - loss_ref) <= 1e-5 * abs(loss_ref)
    for name, p in m.named_parameters():
        e = rel_err(p.grad.cpu().numpy(), ref[name])
        print(precision, (C, G, H, L), name, e)
        assert e <= 2e-5, (name, e)
    assert rel_err(pos_d.grad.cpu().numpy(), pos_ref) <= 2e-5


@pytest.mark.parametrize('C,G,H,L,n', SMALL)
@pytest.mark.parametrize('precision', ['f16x2', 'fp32'])
def test_deterministic_gradients_match_the_oracle(dev, C, G, H, L, n, precision):
    rng = np.random.default_rng(C * 77 + G)
    ds = R.VolumeIndexing((255, 255, 255))
    _, pos = ds.training_positions(torch.from_numpy(rng.integers(0, 255, (n, 3))))
    target = torch.from_numpy(rng.uniform(-1, 1, (n,)).astype(np.float32))
    _parity(dev, C, G, H, L, precision, pos, lambda y, put: torch.nn.functional.mse_loss(y, put(target)))


@pytest.mark.parametrize('precision', ['f16x2', 'fp32'])
def test_headroom_all_samples_in_one_cell(dev, precision):
    """4096 samples at one position: every one of the 8 corner rows receives 4096 contributions of about the same size,
    the case the accumulator's head room (8 n contributions of the maximum) is sized for."""
    n = 4096
    pos = torch.tensor([[0.3, -0.45, 0.1]], dtype=torch.float32).repeat(n, 1)
    target = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (n,)).astype(np.float32))
    _parity(dev, 32, 8, 32, 2, precision, pos, lambda y, put: torch.nn.functional.mse_loss(y, put(target)))


@pytest.mark.parametrize('precision', ['f16x2', 'fp32'])
def test_upstream_gradients_spread_over_fifteen_decades(dev, precision):
    """|g| from 1e-12 to 1e3 in one batch: one quantum per call, taken from the largest feature gradient."""
    n = 1000
    rng = np.random.default_rng(8)
    pos = torch.from_numpy(rng.uniform(-1, 1, (n, 3)).astype(np.float32))
    gv = torch.from_numpy((10.0 ** rng.uniform(-12, 3, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32))
    gv[0], gv[1] = 1e3, -1e-12
    _parity(dev, 32, 8, 32, 2, precision, pos, lambda y, put: (y * put(gv)).sum())


def test_edge_cases_zero_nonfinite_and_workspace(dev):
    from latent_feature_grid_compression_amd import _lib, ops
    C, G, H, L, n = 24, 7, 20, 3, 1000
    m, _ = build_synth(C, G, H, L, seed=3, dev=dev)
    m.train()
    pos = _positions(n, 5).to(dev)
    # zero upstream gradient: exactly zero, no NaN from a 0 / 0
    d_grid = _raw_backward(m, pos, torch.zeros(n, device=dev), True)[0]
    assert int(torch.count_nonzero(d_grid)) == 0 and not bool(torch.isnan(d_grid).any())
    # one NaN and one inf upstream: the WHOLE grid gradient is NaN (the default mode poisons the touched rows only); the
    # weight gradients are those of the default mode bit for bit
    g = torch.from_numpy(np.random.default_rng(1).standard_normal(n).astype(np.float32)).to(dev)
    g[n - 2], g[n - 1] = float('nan'), float('inf')        # samples inside the cube
    assert bool((pos[n - 2:].abs() < 1).all())
    d_grid, d_w, d_b, _ = _raw_backward(m, pos, g, True)
    d_grid_0, d_w0, d_b0, _ = _raw_backward(m, pos, g, False)
    assert bool(torch.isnan(d_grid).all())
    assert bool(torch.isnan(d_grid_0).any()) and not bool(torch.isnan(d_grid_0).all())
    for a, b in zip(d_w + d_b, d_w0 + d_b0):
        assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    for bad in (float('inf'), float('-inf')):              # an infinity alone is enough
        g2 = torch.ones(n, device=dev)
        g2[n - 1] = bad
        assert bool(torch.isnan(_raw_backward(m, pos, g2, True)[0]).all())
    # a workspace one byte short of lfgc_backward_det_workspace_bytes is refused before anything is launched
    lib = _lib.load()
    desc = m._descriptor()
    with torch.no_grad():
        grid_cl, packed = m._decoded_channel_last(), m._packed()
    D, Hh, W, _cs = grid_cl.shape
    y, stash = ops.forward_raw(desc, grid_cl, packed, pos=pos, want_stash=True, precision='fp32')
    need = int(lib.lfgc_backward_det_workspace_bytes(ctypes.byref(desc), n, D, Hh, W))
    assert need > int(lib.lfgc_backward_workspace_bytes(ctypes.byref(desc), n)) + D * Hh * W * 24 * 8
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    ps, _n = ops._positions_struct(pos)
    weights, biases = m._mlp_params()
    dw = [torch.empty_like(w) for w in weights]
    db = [torch.empty_like(b) for b in biases]
    wp, _k1 = _lib.ptr_array([t.data_ptr() for t in dw])
    bp, _k2 = _lib.ptr_array([t.data_ptr() for t in db])
    out = torch.full_like(grid_cl, 7.0)
    rc = lib.lfgc_backward_det_f32(ctypes.byref(desc), ctypes.byref(ps), grid_cl.data_ptr(), D, Hh, W, packed.data_ptr(), 0,
                                   stash.data_ptr(), g.data_ptr(), out.data_ptr(), wp, bp, None, ws.data_ptr(), need - 1, None)
    assert rc == -5
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def _drop_model(kind, wavelet, C, dev):
    from latent_feature_grid_compression_amd.model.model_utils import setup_model
    from latent_feature_grid_compression_amd.model.Dropout_Layer import DropoutLayer
    DropoutLayer.set_threshold_list(None)
    torch.manual_seed(5)
    m = setup_model(3, 32, 1, 2, 'fourier', 2, kind, 0.025, 0.75, wavelet, C, 14, '').to(dev).train()
    assert len(m.feature_grid) >= 3                        # at least two wavelet levels: both adjoint kernels run
    return m


@pytest.mark.parametrize('kind,wavelet,C', [('smallify', 'db2', 6), ('smallify', 'db2', 32), ('smallify', 'haar', 6),
                                            ('smallify', 'haar', 32), ('variational', 'db2', 32)])
def test_pruning_layers_get_bitwise_repeatable_gradients(dev, kind, wavelet, C):
    """Smallify (betas: L1-penalised factors whose gradients ride in the adjoint kernels) on both bases and channel counts
    -- C = 6: one channel group in the channel-last level, 6 slices in the channel-first one; C = 32: 2 and 32 --, and the
    variational layers once with a fixed draw."""
    from latent_feature_grid_compression_amd.model.Smallify_Dropout import SmallifyLoss
    m = _drop_model(kind, wavelet, C, dev)
    torch.manual_seed(9)
    pos = torch.rand(4096, 3, device=dev) * 2 - 1
    if kind == 'variational':
        for d in m.drop:
            d._draw = (lambda xi: (lambda: xi))(torch.randn_like(d.log_thetas))
    crit = SmallifyLoss(weight_l1=1e-3, weight_l2=1e-5)

    def run(flag):
        m.deterministic = flag
        m.zero_grad(set_to_none=True)
        loss = m(pos).square().mean()
        if kind == 'smallify':
            loss = loss + crit(m)
        loss.backward()
        return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}

    run(True)                                              # first step: the loss announces that it consumes the penalty sums
    outs = [run(True) for _ in range(3)]
    plain = run(False)
    want = 'betas' if kind == 'smallify' else 'log_thetas'
    assert sum(want in k for k in outs[0]) == len(m.feature_grid) and set(plain) == set(outs[0])
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[1][k], outs[2][k]), k
        e = rel_err(outs[0][k].cpu().numpy(), plain[k].cpu().numpy())
        assert e <= 1e-5, (k, e)


def _small_train_ctx(dev):
    import bench
    ctx = bench.cfg3_train_setup(dev, 'f16x2', n=4096, vol_shape=(40, 41, 42),
                                 workload=dict(C=16, G=16, H=32, L=2))
    ctx['model'].deterministic = True
    return ctx


def _eager(ctx, steps, keep_at=()):
    losses, kept = [], {}
    for i in range(steps):
        losses.append(ctx['step']().detach().clone())
        if i + 1 in keep_at:
            kept[i + 1] = {k: p.detach().clone() for k, p in ctx['model'].named_parameters()}
    torch.cuda.synchronize()
    return losses, kept


def test_training_runs_are_bit_identical_eager_and_graph_replayed(dev):
    """Two models from the same seed, the device lattice sampler at the same seed, Adam(lr = 0.008): after five steps all
    parameters and the five losses are equal bit for bit.  Then one such step captured in a HIP graph (bench.py's
    sequence: 3 eager warm-up steps, capture, replays): 5 replays leave the parameters and write the losses of the 8 eager
    steps, bit for bit."""
    import bench
    K, warm = 5, 3
    losses_x, kept_x = _eager(_small_train_ctx(dev), warm + K, keep_at=(K, warm + K))
    ctx_y = _small_train_ctx(dev)
    losses_y, _ = _eager(ctx_y, K)
    for a, b in zip(losses_x[:K], losses_y):
        assert torch.equal(a, b)
    moved = 0.0
    for k, p in ctx_y['model'].named_parameters():
        assert torch.equal(p.detach(), kept_x[K][k]), k
    assert len({float(l) for l in losses_x}) == warm + K                # the batches (and the model) really change

    ctx_g = _small_train_ctx(dev)
    start = {k: p.detach().clone() for k, p in ctx_g['model'].named_parameters()}
    graph, loss_g, eager_g = bench.capture_train_step(ctx_g, eager_warmup=warm)
    replayed = []
    for _ in range(K):
        graph.replay()
        torch.cuda.synchronize()
        replayed.append(loss_g.detach().clone())
    assert ctx_g['ds']._sample_state.cpu().tolist() == [warm + K, 0]
    for a, b in zip(eager_g + replayed, losses_x):
        assert torch.equal(a, b), (float(a), float(b))
    for k, p in ctx_g['model'].named_parameters():
        assert torch.equal(p.detach(), kept_x[warm + K][k]), k
        moved = max(moved, float((p.detach() - start[k]).abs().max()))
    assert moved > 0.008
