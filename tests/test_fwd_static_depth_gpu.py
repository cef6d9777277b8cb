"""The f16 inference kernels compile their tile body for the net's depth where that depth is 4 (csrc/lfgc_forward16.h,
template parameter LD: four layers written out straight-line, ring slots and DMA plans folded to constants).  The
any-depth body is still there (`LFGC_FWD_RUNTIME_DEPTH=1` forces it) and runs every other depth.  The specialised body
executes the same arithmetic in the same order, so for a 4-layer net it must return the BITS of the any-depth body:
HIP against HIP is torch.equal, and each of the two is within the project's 1e-5 of oracle/ref_torch.py, measured as
tests/test_hip_forward.py measures it (largest error over largest reference value).  The single-product mode (`f16`)
is no fp32-level mode: one f16 rounding (2^-11) per operand, 2.2e-4 to 6.1e-4 on these cases, so against the oracle it
is held to the 3e-3 that tests/test_hip_forward.py states for it, and to torch.equal between the two bodies like the rest.

Streamed family (32 channels, 128 wide) on a non-cubic 12 x 16 x 20-cell grid: lattices 5 x 6 x 96 (three whole
32-voxel runs per row; 90 tiles, so the last 8-wave batch holds tiles past the end) and 5 x 6 x 80 (a ragged last run),
with 8- and 4-wave workgroups, hi/lo split and single product; the same net on 4 097 positions from U(-1.05, 1.05)^3
(per-sample gather, a partial tile, corners outside the grid).  Resident family (16 channels, 64 wide): lattice
7 x 9 x 64.  Depths 2, 3 and 5 must still match the oracle: they run the any-depth body whatever the switch says."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_forward import build_synth, rel_err, dev  # noqa: F401

pytestmark = pytest.mark.gpu

GRID = (12, 16, 20)                       # (D, H, W) cells
LATTICES = ((5, 6, 96), (5, 6, 80))
N_POS = 4097
# against the oracle: the project's 1e-5 for the hi/lo split (the default arithmetic); the single-product mode carries one
# f16 rounding (2^-11) per operand through the layers and is held to the bound tests/test_hip_forward.py states for it
TOL = {'f16x2': 1e-5, 'f16': 3e-3}

_models, _refs = {}, {}


def _model(key, dev):
    """key = (C, H, L, grid_shape or cube edge)"""
    if key not in _models:
        C, H, L, g = key
        if isinstance(g, tuple):
            m, sm = build_synth(C, max(g), H, L, seed=8100 + 10 * L + C, dev=dev, grid_shape=g)
        else:
            m, sm = build_synth(C, g, H, L, seed=8100 + 10 * L + C, dev=dev)
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        dense = R.decode_volume(sm['coeffs'], sm['shape_array'], sm['filter_rev'])
        _models[key] = (m.eval(), sm, dense)
    return _models[key]


def _lattice_ref(key, res, dev):
    """The oracle on the reference's own tile positions, once per (net, lattice); never written to afterwards."""
    if (key, res) not in _refs:
        _m, sm, dense = _model(key, dev)
        rds = R.VolumeIndexing(res)
        ref = torch.empty(res)
        for b in R.tile_iter(rds.vol_res_touple, 32):
            yt = R.forward_from_grid(dense, sm['weights'], sm['biases'], R.tile_positions(rds, b).reshape(-1, 3), 2).clamp(-1, 1)
            ref[b[0]:b[1], b[2]:b[3], b[4]:b[5]] = yt.reshape(b[1] - b[0], b[3] - b[2], b[5] - b[4])
        _refs[(key, res)] = ref.numpy()
    return _refs[(key, res)]


class _env:
    """Environment switches of the forward entry for the duration of a block."""

    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        for k, v in self.kv.items():
            os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k in self.kv:
            os.environ.pop(k, None)


def _both_depth_arms(run):
    """run() with the depth-specialised kernel (default) and with the any-depth one -> (specialised, runtime)"""
    spec = run()
    with _env(LFGC_FWD_RUNTIME_DEPTH=1):
        runtime = run()
    return spec, runtime


def _run_lattice(m, res, precision, expect, zrun=1):
    from latent_feature_grid_compression_amd import ops
    lattice = (res, 0, res[0], 32)
    with torch.no_grad():
        grid_cl = m._decoded_channel_last()
        plan = ops.forward_plan(m._descriptor(), grid_cl, lattice=lattice)
        assert (plan.CH, plan.MT, plan.resident, plan.waves) == expect, (plan.CH, plan.MT, plan.resident, plan.waves)
        assert plan.zrun == zrun
        y, _ = ops.forward_raw(m._descriptor(), grid_cl, m._packed(), lattice=lattice, clamp=True, precision=precision)
    torch.cuda.synchronize()
    return y.view(res).cpu()


@pytest.mark.parametrize('precision', ['f16x2', 'f16'])
@pytest.mark.parametrize('waves', [8, 4])
@pytest.mark.parametrize('res', LATTICES, ids=lambda r: 'x'.join(map(str, r)))
def test_streamed_lattice_bits_equal_the_runtime_depth_kernel(dev, res, waves, precision):
    key = (32, 128, 4, GRID)
    m, _sm, _dense = _model(key, dev)
    with _env(LFGC_FWD_WAVES=waves):
        spec, runtime = _both_depth_arms(lambda: _run_lattice(m, res, precision, (32, 4, 0, waves)))
    ref = _lattice_ref(key, res, dev)
    tol = TOL[precision]
    for arm, y in (('specialised', spec), ('runtime', runtime)):
        e = rel_err(y.numpy(), ref)
        print('STATIC-DEPTH lattice %s waves %d %s %s | vs oracle %.3e' % ('x'.join(map(str, res)), waves, precision, arm, e))
        assert np.isfinite(y.numpy()).all()
        assert e <= tol, (arm, e)
    assert torch.equal(spec, runtime), 'the depth-specialised kernel does not return the any-depth kernel\'s bits'


@pytest.mark.parametrize('precision', ['f16x2', 'f16'])
def test_position_list_bits_equal_the_runtime_depth_kernel(dev, precision):
    from latent_feature_grid_compression_amd import ops
    key = (32, 128, 4, GRID)
    m, sm, dense = _model(key, dev)
    rng = np.random.default_rng(8200)
    pos = torch.from_numpy(rng.uniform(-1.05, 1.05, (N_POS, 3)).astype(np.float32))
    pos_d = pos.to(dev)

    def run():
        with torch.no_grad():
            grid_cl = m._decoded_channel_last()
            plan = ops.forward_plan(m._descriptor(), grid_cl, pos=pos_d)
            assert (plan.CH, plan.MT, plan.resident, plan.zrun) == (32, 4, 0, 0)
            y, _ = ops.forward_raw(m._descriptor(), grid_cl, m._packed(), pos=pos_d, precision=precision)
        torch.cuda.synchronize()
        return y.cpu()

    spec, runtime = _both_depth_arms(run)
    ref = R.forward_from_grid(dense, sm['weights'], sm['biases'], pos, 2).numpy()
    for arm, y in (('specialised', spec), ('runtime', runtime)):
        e = rel_err(y.numpy(), ref)
        print('STATIC-DEPTH positions n%d %s %s | vs oracle %.3e' % (N_POS, precision, arm, e))
        assert np.isfinite(y.numpy()).all()
        assert e <= TOL[precision], (arm, e)
    assert torch.equal(spec, runtime), 'the depth-specialised kernel does not return the any-depth kernel\'s bits'


@pytest.mark.parametrize('precision', ['f16x2', 'f16'])
def test_resident_lattice_bits_equal_the_runtime_depth_kernel(dev, precision):
    key, res = (16, 64, 4, 8), (7, 9, 64)
    m, _sm, _dense = _model(key, dev)
    spec, runtime = _both_depth_arms(lambda: _run_lattice(m, res, precision, (16, 2, 1, 4)))
    ref = _lattice_ref(key, res, dev)
    for arm, y in (('specialised', spec), ('runtime', runtime)):
        e = rel_err(y.numpy(), ref)
        print('STATIC-DEPTH resident lattice 7x9x64 %s %s | vs oracle %.3e' % (precision, arm, e))
        assert np.isfinite(y.numpy()).all()
        assert e <= TOL[precision], (arm, e)
    assert torch.equal(spec, runtime), 'the depth-specialised kernel does not return the any-depth kernel\'s bits'


@pytest.mark.parametrize('L', [2, 3, 5])
def test_other_depths_run_the_any_depth_kernel(dev, L):
    """Depths other than 4 are not sent to the 4-layer body (which would read layer blocks that do not exist or stop
    short): they match the oracle, and the switch changes nothing for them."""
    key, res = (32, 128, L, GRID), LATTICES[0]
    m, _sm, _dense = _model(key, dev)
    default, forced = _both_depth_arms(lambda: _run_lattice(m, res, 'f16x2', (32, 4, 0, 4)))
    e = rel_err(default.numpy(), _lattice_ref(key, res, dev))
    print('STATIC-DEPTH selection L%d lattice %s | vs oracle %.3e' % (L, 'x'.join(map(str, res)), e))
    assert e <= 1e-5, e
    assert torch.equal(default, forced)


@pytest.mark.parametrize('key,res,expect', [
    ((32, 128, 4, GRID), LATTICES[0], (32, 4, 0, 4)),
    ((32, 128, 4, GRID), LATTICES[1], (32, 4, 0, 4)),
    ((16, 64, 4, 8), (7, 9, 64), (16, 2, 1, 4)),
], ids=['5x6x96', '5x6x80', 'resident-7x9x64'])
def test_lattices_above_take_the_zrun_path(dev, key, res, expect):
    """The relation tests/fuzz_zrun.py sweeps: where the plan says z-run tiles + column sampler, the result agrees with the
    per-sample gather (`LFGC_NO_ZRUN=1`) to 3e-6 of the largest output -- the same trilinear sum in another order.  The
    plan must say z-run on every lattice of this file, so the equality tests above do exercise the column sampler."""
    m, _sm, _dense = _model(key, dev)
    zrun = _run_lattice(m, res, 'f16x2', expect, zrun=1)
    with _env(LFGC_NO_ZRUN=1):
        gather = _run_lattice(m, res, 'f16x2', expect, zrun=0)
    e = rel_err(zrun.numpy(), gather.numpy())
    print('STATIC-DEPTH sampler %s | z-run vs gather %.3e' % ('x'.join(map(str, res)), e))
    assert e <= 3e-6, e
