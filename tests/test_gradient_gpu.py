"""GPU tests of the input-gradient path: d output / d position without the parameter gradients.

lfgc_input_gradient_f32 (the INPUT_ONLY build of the backward data kernel), the slab-position kernel,
Feature_Grid_Model.value_and_gradient and the volume drivers of visualization/OutputToVTK.py, against the reference
fixtures (tests/golden) and the oracle's autograd.  Bounds are the project's own for position gradients
(tests/test_hip_backward.py): max|g - ref| / max|ref| <= 2e-5 for 'fp32' and 'f16x2', 3e-2 for the reduced 'f16' build.

The trilinear derivative jumps at cell faces, so gradients are only ever compared at bit-identical fp32 positions: the
oracle is always handed the very tensor the device used (the kernel follows ATen's fp32 arithmetic op for op and lands
on ATen's side of a face)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_forward import build_from_golden, build_synth, rel_err, GOLD, dev  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = {'fp32': 2e-5, 'f16x2': 2e-5, 'f16': 3e-2}


def _oracle(m):
    """pos (N,3) CPU -> (y (N,) unclamped, d sum(y) / d pos (N,3)) by the oracle's autograd on the model's parameters."""
    coeffs = [p.detach().cpu() for p in m.feature_grid]
    layers = list(m.net_layers) + [m.final_layer]
    ws, bs = [l.weight.detach().cpu() for l in layers], [l.bias.detach().cpu() for l in layers]
    dense = R.decode_volume(coeffs, m.shape_array, m.filter.filter_rev.detach().cpu())

    def run(pos, d_out=None):
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        p = pos.detach().cpu().clone().requires_grad_(True)
        y = R.forward_from_grid(dense, ws, bs, p, m.n_freqs).squeeze(-1)
        (y.sum() if d_out is None else (y * d_out).sum()).backward()
        return y.detach().numpy(), p.grad.numpy()
    return run


def _raw(m):
    with torch.no_grad():
        return m._descriptor(), m._decoded_channel_last(), m._packed()


def _test_positions(G, n, seed):
    """n lattice points of a 255^3 volume (the backward tests' positions) + 64 hard ones: exactly +-1, beyond +-1 (zero
    padding: no sampler gradient) and on the centres of the grid's cells (where the sampler's floor() lands on a face)."""
    rng = np.random.default_rng(seed)
    ds = R.VolumeIndexing((255, 255, 255))
    _, pos = ds.training_positions(torch.from_numpy(rng.integers(0, 255, (n, 3))))
    extra = rng.uniform(-1, 1, (64, 3)).astype(np.float32)
    for i in range(16):                                   # exactly +-1 on one, two or all three axes
        axes = rng.permutation(3)[:1 + i % 3]
        extra[i, axes] = rng.choice([-1.0, 1.0], len(axes))
    for i in range(16, 32):                               # beyond +-1
        axes = rng.permutation(3)[:1 + i % 3]
        extra[i, axes] = rng.choice([-3.0, -1.5, -1.001, 1.001, 1.5, 3.0], len(axes))
    centres = (2 * rng.integers(0, G, (32, 3)) + 1).astype(np.float32) / np.float32(G) - np.float32(1)
    extra[32:] = centres
    return torch.cat([pos, torch.from_numpy(extra)], 0).contiguous()


def _gradient(m, pos_d, precision, d_out=None, out=None):
    from latent_feature_grid_compression_amd import ops
    desc, grid_cl, packed = _raw(m)
    y, stash = ops.forward_raw(desc, grid_cl, packed, pos=pos_d, want_stash=True, precision=precision)
    return y, ops.input_gradient_raw(desc, grid_cl, packed, pos_d, stash, d_out=d_out, precision=precision, out=out)


# ---- 1. reference fixtures ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['fp32', 'f16x2'])
@pytest.mark.parametrize('name', ['fwd_c4g15h16l3.npz', 'fwd_c6g17h32l4.npz'])
def test_input_gradient_matches_reference_fixture(dev, name, precision):
    """d loss / d pos of the reference's own autograd (mse loss, positions marked requires_grad as training.py:99 does):
    the forward's y gives d_out = 2 (y - target) / N, the new entry the rest."""
    g = np.load(os.path.join(GOLD, name))
    m = build_from_golden(g, dev).train()
    pos = torch.from_numpy(g['pos']).to(dev)
    target = torch.from_numpy(g['target']).to(dev)
    from latent_feature_grid_compression_amd import ops
    desc, grid_cl, packed = _raw(m)
    y, stash = ops.forward_raw(desc, grid_cl, packed, pos=pos, want_stash=True, precision=precision)
    d_out = 2.0 * (y - target) / y.numel()
    got = ops.input_gradient_raw(desc, grid_cl, packed, pos, stash, d_out=d_out, precision=precision)
    err = rel_err(got.cpu().numpy(), g['grad_pos'])
    print('%s %s: rel err %.3e' % (name, precision, err))
    assert err <= 2e-5


# ---- 2. / 3. every compiled instantiation against the oracle ---------------------------------------------------------

_MATRIX = [(C, 8, H, 2) for C in (5, 16, 22, 32) for H in (20, 64, 128)] + [(3, 15, 100, 1), (5, 4, 4, 2)]
_REF = {}


def _model_and_reference(shape, n, dev_, tag):
    """(model, positions on the device, oracle y, oracle gradient), built once per shape and shared by the precisions."""
    key = (shape, n, tag)
    if key not in _REF:
        C, G, H, L = shape
        m, _ = build_synth(C, G, H, L, seed=6000 + C + G + H, dev=dev_)
        m.train()
        pos = _test_positions(G, n, seed=C * 131 + H)
        y_ref, g_ref = _oracle(m)(pos)
        _REF.clear()                                        # one shape at a time: the parametrisation runs shape-major
        _REF[key] = (m, pos.to(dev_), y_ref, g_ref)
    return _REF[key]


@pytest.mark.parametrize('precision', ['fp32', 'f16x2', 'f16'])
@pytest.mark.parametrize('shape', _MATRIX, ids=lambda s: 'C%dG%dH%dL%d' % s)
def test_input_gradient_kernel_matrix(dev, shape, precision):
    """CH 8/16/24/32 x MT 1/2/4 and the backward tests' two odd shapes, 4-wave workgroups, d_out = None (ones): the
    gradient of the output itself against the oracle's autograd of y.sum() at the same fp32 positions."""
    from latent_feature_grid_compression_amd import ops
    m, pos_d, _y_ref, g_ref = _model_and_reference(shape, 300, dev, 'w4')
    plan = ops.input_gradient_plan(m._descriptor(), pos_d.shape[0], precision)
    assert plan.waves == 4 and plan.nslabs == 0 and plan.roles == 0
    assert (plan.CH, plan.MT) == ((shape[0] + 7) // 8 * 8, {1: 1, 2: 2, 3: 4, 4: 4}[(shape[2] + 31) // 32])
    _, got = _gradient(m, pos_d, precision)
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    err = rel_err(got, g_ref)
    print('C%d G%d H%d L%d %s: rel err %.3e' % (shape + (precision, err)))
    assert err <= TOL[precision]


@pytest.mark.parametrize('precision', ['fp32', 'f16x2', 'f16'])
@pytest.mark.parametrize('waves', [8, 4])
@pytest.mark.parametrize('C', [5, 16, 22, 32])
def test_input_gradient_many_batches(dev, C, waves, precision):
    """Workgroups that walk more than one batch -- the ring's hand-over across the batch boundary, which the training
    build's staging barrier used to cover -- with a ragged last tile.  waves = 8: a 256-sample batch for every CU and 77
    samples more.  waves = 4: one 256-sample group short of that, so 4-wave workgroups take two 128-sample batches."""
    from latent_feature_grid_compression_amd import ops
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    desc = ops.make_desc(C, 128, 2, 2)
    if ops.input_gradient_plan(desc, 256 * cus, precision).waves != 8:          # take the CU count from the plan's own rule
        cus = ops.input_gradient_plan(desc, 1 << 30, precision).grid
    n = 256 * cus + 77 if waves == 8 else 256 * (cus - 1) - 51
    plan = ops.input_gradient_plan(desc, n, precision)
    assert plan.waves == waves and plan.nbatches > plan.grid
    m, pos_d, _y_ref, g_ref = _model_and_reference((C, 8, 128, 2), n - 64, dev, 'w%d' % waves)
    assert pos_d.shape[0] == n
    _, got = _gradient(m, pos_d, precision)
    err = rel_err(got.cpu().numpy(), g_ref)
    print('C%d H128 L2 n=%d waves=%d %s: rel err %.3e' % (C, n, waves, precision, err))
    assert err <= TOL[precision]


# ---- 4. ragged sizes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape,resident', [((8, 8, 32, 2), 1), ((32, 8, 128, 4), 0)], ids=['resident', 'streamed'])
def test_ragged_sizes_leave_the_rows_past_n_alone(dev, shape, resident):
    from latent_feature_grid_compression_amd import ops
    C, G, H, L = shape
    m, _ = build_synth(C, G, H, L, seed=6100 + C, dev=dev)
    m.train()
    desc, grid_cl, _packed = _raw(m)
    oracle = _oracle(m)
    pos_all = _test_positions(G, 257 - 64, seed=9)
    g_all = oracle(pos_all)[1]
    for n in (1, 31, 32, 33, 257):
        pos_d = pos_all[:n].contiguous().to(dev)
        assert ops.forward_plan(desc, grid_cl, pos=pos_d, want_stash=True).resident == resident
        buf = torch.full((n + 64, 3), -777.25, dtype=torch.float32, device=dev)
        _gradient(m, pos_d, 'f16x2', out=buf[:n])
        assert torch.equal(buf[n:], torch.full((64, 3), -777.25, dtype=torch.float32, device=dev)), n
        assert rel_err(buf[:n].cpu().numpy(), g_all[:n]) <= 2e-5, n


# ---- 5. the model's API ----------------------------------------------------------------------------------------------------

def test_value_and_gradient_builds_no_graph(dev):
    """Train mode, eval mode, under no_grad and with an eval-shaped input: afterwards no parameter has a .grad, the outputs
    carry no graph, and forward returns the bits it returned before."""
    g = np.load(os.path.join(GOLD, 'fwd_c4g15h16l3.npz'))
    m = build_from_golden(g, dev)
    oracle = _oracle(m)
    flat = torch.from_numpy(g['pos']).to(dev)
    tile = torch.from_numpy(g['eval_pos']).to(dev)                        # (1, 1, 8, 9, 10, 3)
    for training, pos, no_grad in ((True, flat, False), (True, flat, True), (False, flat, False), (False, tile, False),
                                   (False, tile, True)):
        m.train(training)
        with torch.no_grad():
            before = m(pos).clone()
        if no_grad:
            with torch.no_grad():
                value, grad = m.value_and_gradient(pos)
        else:
            value, grad = m.value_and_gradient(pos)
        assert all(p.grad is None for p in m.parameters())
        assert not value.requires_grad and not grad.requires_grad and value.grad_fn is None and grad.grad_fn is None
        assert grad.shape == pos.shape and value.shape == before.shape
        assert torch.equal(value, before)                                 # the value forward gives in that mode
        with torch.no_grad():
            assert torch.equal(m(pos), before)
        y_ref, g_ref = oracle(pos.reshape(-1, 3))
        assert rel_err(grad.reshape(-1, 3).cpu().numpy(), g_ref) <= 2e-5
        if tuple(pos.shape) == tuple(tile.shape):
            assert rel_err(value.cpu().numpy(), np.clip(y_ref, -1, 1)) <= 1e-5
    m.train()
    with pytest.raises(ValueError):
        m.value_and_gradient(tile)                                        # (N, 3) only in training mode, as forward


def test_gradient_is_of_the_unclamped_output(dev):
    """Eval mode clamps the value to [-1, 1]; the gradient stays that of the unclamped output where the value saturates."""
    m, _ = build_synth(16, 8, 64, 2, seed=6200, dev=dev)
    pos = _test_positions(8, 1000, seed=3).to(dev)
    scale = 1.0 / float(np.median(np.abs(_oracle(m)(pos)[0])))           # the output is linear in the final layer: half the
    with torch.no_grad():                                                 # samples end up beyond +-1
        m.final_layer.weight.mul_(scale)
        m.final_layer.bias.mul_(scale)
    m.eval()
    y_ref, g_ref = _oracle(m)(pos)
    saturated = np.abs(y_ref) > 1.0
    assert 50 < saturated.sum() < saturated.size                          # both kinds of sample are present
    value, grad = m.value_and_gradient(pos)
    with torch.no_grad():
        assert torch.equal(value, m(pos))
    v = value.reshape(-1).cpu().numpy()
    assert np.abs(v).max() == 1.0 and rel_err(v, np.clip(y_ref, -1, 1)) <= 1e-5
    got = grad.cpu().numpy()
    assert (np.abs(got[saturated]).max(axis=1) > 0).all()
    assert rel_err(got[saturated], g_ref[saturated]) <= 2e-5 and rel_err(got, g_ref) <= 2e-5


@pytest.mark.parametrize('precision', ['fp32', 'f16x2'])
def test_chunked_runs_are_the_single_run(dev, precision):
    """A stash budget of one 256-sample group forces 6 chunks.  'fp32' is per-sample arithmetic: bit-equal.  'f16x2' scales
    the gradients per 32-sample tile; chunks are multiples of 256, so tiles keep their members: within 2e-5, and bit-equal
    too on every run so far (printed)."""
    from latent_feature_grid_compression_amd import _lib, ops
    m, _ = build_synth(16, 8, 64, 2, seed=6300, dev=dev)
    m.eval()
    m.precision = precision
    pos = _test_positions(8, 5 * 256 + 100 - 64, seed=4).to(dev)
    per = int(_lib.load().lfgc_stash_bytes(ctypes.byref(m._descriptor()), 256))
    assert -(-pos.shape[0] // ops.gradient_chunk_samples(m._descriptor(), pos.shape[0], per)) >= 5
    v1, g1 = m.value_and_gradient(pos)
    v6, g6 = m.value_and_gradient(pos, max_stash_bytes=per)
    print('%s: chunked == single run bit for bit: %s' % (precision, torch.equal(g1, g6)))
    assert torch.equal(v1, v6)
    if precision == 'fp32':
        assert torch.equal(g1, g6)
    assert rel_err(g6.cpu().numpy(), g1.cpu().numpy()) <= 2e-5


@pytest.mark.parametrize('precision', ['fp32', 'f16x2'])
def test_agrees_with_the_autograd_route(dev, precision):
    """pos.requires_grad_() + m.train()(pos).sum().backward() runs the training build of the same kernel."""
    m, _ = build_synth(22, 8, 64, 3, seed=6400, dev=dev)
    m.train()
    m.precision = precision
    pos = _test_positions(8, 3000, seed=5).to(dev)
    p = pos.clone().requires_grad_(True)
    m(p).sum().backward()
    m.zero_grad(set_to_none=True)
    value, grad = m.value_and_gradient(pos)
    diff = (grad - p.grad).abs().max().item()
    print('%s: max |value_and_gradient - autograd route| = %.3e (largest entry %.3e)' % (precision, diff, p.grad.abs().max().item()))
    assert rel_err(grad.cpu().numpy(), p.grad.cpu().numpy()) <= 2e-5


# ---- 6. range safety ----------------------------------------------------------------------------------------------------------

def test_gradient_is_range_safe(dev):
    """Grid features of 4e5 leave the f16 range (the case of test_default_precision_is_range_safe): the forward's exact redo
    rewrites the stash, and the gradient comes out finite and reference-equivalent under the default precision."""
    C, G, H, L = 16, 16, 64, 4
    m, _ = build_synth(C, G, H, L, seed=77, dev=dev)
    with torch.no_grad():
        for p in m.feature_grid:
            p.mul_(4.0e5)
        m.net_layers[0].weight[:, 15:].mul_(2.5e-6)
    m.train()
    assert m.precision == 'f16x2'
    rng = np.random.default_rng(5)
    pos = torch.from_numpy(rng.uniform(-1, 1, (3000, 3)).astype(np.float32))
    y_ref, g_ref = _oracle(m)(pos)
    value, grad = m.value_and_gradient(pos.to(dev))
    got = grad.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(g_ref).all()
    assert rel_err(value.reshape(-1).cpu().numpy(), y_ref) <= 1e-5
    err = rel_err(got, g_ref)
    print('range case: rel err %.3e' % err)
    assert err <= 2e-5


# ---- 7. slab positions -------------------------------------------------------------------------------------------------------

def _tile_positions_volume(res):
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    from latent_feature_grid_compression_amd.visualization.OutputToVTK import iter_tiles
    ds = IndexDataset(res, 16, build_index_table=False)
    want = torch.zeros(res + (3,))
    for (x0, x1, y0, y1, z0, z1) in iter_tiles(res, 32):
        want[x0:x1, y0:y1, z0:z1] = ds.tile_positions((x0, y0, z0), (x1, y1, z1))
    return ds, want


@pytest.mark.parametrize('res', [(70, 40, 33), (37, 20, 33)])
def test_slab_positions_are_the_tile_positions(dev, res):
    """lfgc_lattice_slab_positions_f32 against IndexDataset.tile_positions assembled over iter_tiles (33 = 32 + 1: a
    one-voxel tile), bound: max |difference| <= 6e-8, one fp32 ulp below 1.  Bit-equality is expected on a host whose
    torch.linspace contracts start + step * i into a fused multiply-add (every x86 host with FMA units), as the device
    function does, and is printed; a host without it differs by one linspace ulp doubled, 1.2e-7, at a few voxels."""
    from latent_feature_grid_compression_amd import ops
    ds, want = _tile_positions_volume(res)
    full = ops.lattice_slab_positions(res, 0, res[0], 32, ds.scales.tolist(), dev)
    assert full.shape == (res[0] * res[1] * res[2], 3)
    got = full.view(res + (3,)).cpu()
    diff = (got - want).abs().max().item()
    print('res %s: max |kernel - tile_positions| = %.3e, bit-equal: %s' % (res, diff, torch.equal(got, want)))
    assert diff <= 6e-8


def test_slab_positions_are_the_reference_s_recorded_tiles(dev):
    """The twelve tile position tensors the reference's own driver formed for the 70 x 40 x 33 volume
    (tests/golden/tiles_70x40x33.npz), independent of the host this test runs on: bit for bit."""
    from latent_feature_grid_compression_amd import ops
    from latent_feature_grid_compression_amd.visualization.OutputToVTK import iter_tiles
    g = np.load(os.path.join(GOLD, 'tiles_70x40x33.npz'))
    res = (70, 40, 33)
    got = ops.lattice_slab_positions(res, 0, 70, 32, g['scales'].tolist(), dev).view(res + (3,)).cpu().numpy()
    for t, (x0, x1, y0, y1, z0, z1) in enumerate(iter_tiles(res, 32)):
        assert np.array_equal(got[x0:x1, y0:y1, z0:z1], g['tile%d' % t][0]), t


@pytest.mark.parametrize('res', [(70, 40, 33), (37, 20, 33)])
def test_slab_positions_are_the_fused_forward_s_lattice(dev, res):
    """What the drivers rely on: a slab is the same rows of the full range ([32, 70) cut to the volume, [32, 37) for the
    37-voxel one), and the positions are the ones the fused forward forms for itself in lattice mode -- the exact build
    evaluated at them returns the bits of its lattice-mode pass."""
    from latent_feature_grid_compression_amd import ops
    ds, _want = _tile_positions_volume(res)
    scales = ds.scales.tolist()
    full = ops.lattice_slab_positions(res, 0, res[0], 32, scales, dev)
    xe = min(70, res[0])
    part = ops.lattice_slab_positions(res, 32, xe, 32, scales, dev)
    assert torch.equal(part.view(xe - 32, res[1], res[2], 3), full.view(res + (3,))[32:xe])
    m, _ = build_synth(8, 8, 32, 2, seed=6600, dev=dev)
    desc, grid_cl, packed = _raw(m)
    y_lattice, _ = ops.forward_raw(desc, grid_cl, packed, lattice=(res, 32, xe, 32), precision='fp32')
    y_explicit, _ = ops.forward_raw(desc, grid_cl, packed, pos=part, precision='fp32')
    assert torch.equal(y_lattice, y_explicit)


# ---- 8. volume drivers -------------------------------------------------------------------------------------------------------

def test_gradient_volume_drivers(dev):
    from latent_feature_grid_compression_amd import ops
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    from latent_feature_grid_compression_amd.data.Interpolation import finite_difference_trilinear_grad
    from latent_feature_grid_compression_amd.visualization import OutputToVTK as V
    g = np.load(os.path.join(GOLD, 'tiles_70x40x33.npz'))
    m = build_from_golden(np.load(os.path.join(GOLD, 'fwd_c4g15h16l3.npz')), dev).eval()
    ds = IndexDataset(torch.from_numpy(g['volume']), 16, build_index_table=False)
    res = ds.vol_res_touple
    full = V.gradient_field_from_net(ds, m)
    assert full.shape == res + (3,) and full.is_cuda
    pos = ops.lattice_slab_positions(res, 0, res[0], 32, ds.scales.tolist(), dev)
    _, g_ref = _oracle(m)(pos)                                  # at the positions the device used
    err = rel_err(full.view(-1, 3).cpu().numpy(), g_ref)
    print('volume gradient: rel err %.3e' % err)
    assert err <= 2e-5
    assert torch.equal(V.gradient_field_from_net(ds, m, 32, 70), full[32:70])
    # several chunks of whole x-rows (a stash budget of a few rows) give the same field
    row_bytes = ops._lib.load().lfgc_stash_bytes(ctypes.byref(m._descriptor()), res[1] * res[2])
    assert torch.equal(V.gradient_field_from_net(ds, m, max_stash_bytes=9 * int(row_bytes)), full)
    out = torch.empty(res + (3,), dtype=torch.float32, device=dev)
    assert V.gradient_field_from_net(ds, m, out=out, index_units=True) is out
    assert torch.equal(out, full * V.index_units_factor(ds)) and V.index_units_factor(ds) == 2.0 / float(ds.max_dim)
    assert all(p.grad is None for p in m.parameters())

    # statistics against the finite differences of a ground-truth volume that is affine in the voxel index
    i, j, k = torch.meshgrid(*[torch.arange(r, dtype=torch.float32) for r in res], indexing='ij')
    slopes = (0.004, -0.007, 0.011)
    vol = (slopes[0] * i + slopes[1] * j + slopes[2] * k - 0.3).to(dev)
    stats = V.gradient_deviation_statistics(ds, m, vol)
    assert len(stats) == 4 and all(np.isfinite(s) for s in stats)
    few = V.gradient_deviation_statistics(ds, m, vol, max_stash_bytes=9 * int(row_bytes))
    assert np.allclose(few, stats, rtol=1e-9)                   # fp64 partial sums, chunked differently
    raw = torch.stack([i, j, k], -1)[32:70].reshape(-1, 3).to(dev)
    direct = finite_difference_trilinear_grad(raw, vol, ds.min_idx, ds.max_idx, ds.vol_res, scale=ds.scales)
    gt = V.gradient_ground_truth(ds, vol, 32, 70)
    assert torch.equal(gt, direct)
    # its units are the network gradient's: d vol / d (normalised position) = slope per voxel / (2 / max_dim)
    want = torch.tensor(slopes, device=dev) / V.index_units_factor(ds)
    assert (gt - want).abs().max().item() <= 1e-3 * want.abs().max().item()
    # and the statistics are those of the two fields
    gt_full = V.gradient_ground_truth(ds, vol)
    mse = ((gt_full - full.view(-1, 3)).double() ** 2).mean().item()
    assert abs(stats[2] - mse) <= 1e-6 * mse


# ---- 9. graph capture ----------------------------------------------------------------------------------------------------------

def test_chunk_is_graph_capturable(dev):
    """One chunk -- forward with stash + input gradient on preallocated tensors -- captured and replayed twice: the bits
    of the eager run (no workspace, no allocation, no synchronisation inside the entry)."""
    from latent_feature_grid_compression_amd import _lib, ops
    m, _ = build_synth(16, 8, 64, 2, seed=6500, dev=dev)
    m.eval()
    desc, grid_cl, packed = _raw(m)
    pos = _test_positions(8, 1000, seed=6).to(dev)
    n = pos.shape[0]
    stash = torch.empty(int(_lib.load().lfgc_stash_bytes(ctypes.byref(desc), n)) // 4, dtype=torch.float32, device=dev)
    y, grad = torch.empty(n, device=dev), torch.empty((n, 3), device=dev)

    def chunk():
        ops.forward_raw(desc, grid_cl, packed, pos=pos, want_stash=True, out=y, stash=stash)
        ops.input_gradient_raw(desc, grid_cl, packed, pos, stash, out=grad)

    chunk()
    torch.cuda.synchronize()
    y0, g0 = y.clone(), grad.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chunk()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chunk()
    for _ in range(2):
        y.zero_()
        grad.fill_(float('nan'))
        stash.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, y0) and torch.equal(grad, g0)
