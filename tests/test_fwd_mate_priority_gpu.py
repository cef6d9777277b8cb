"""The 8-wave streamed forward kernels hand issue priority between the two waves of a SIMD inside every layer
(csrc/lfgc_forward16.h, lfgc_mate_prio).  Priority orders instruction issue and nothing else, so the 8-wave kernel must
return the bits of the 4-wave kernel, which has one wave per SIMD and no priority pattern: HIP against HIP is
torch.equal, outputs and stash, and each of the two is within the project's 1e-5 of oracle/ref_torch.py.

Streamed net (32 channels, 128 wide) on an 8^3 grid with 2, 3, 4 and 5 hidden layers -- the layer chain's pair loop and
both of its tail branches -- in lattice mode through the z-run column sampler and through the per-sample gather
(`LFGC_NO_ZRUN=1`), and as a position list with a stash.  Lattices: 16 x 16 x 64 (two whole 32-voxel runs per row),
16 x 16 x 40 (a ragged second run) and 5 x 7 x 40 (70 tiles: the last 8-wave batch holds tiles past the end)."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_torch as R
from test_hip_forward import build_synth, rel_err, dev  # noqa: F401
from test_kernel_matrix_gpu import _stash_live

pytestmark = pytest.mark.gpu

C, G, H = 32, 8, 128
LAYERS = (2, 3, 4, 5)
LATTICES = ((16, 16, 64), (16, 16, 40), (5, 7, 40))
N_POS = 4096 + 17

_models, _refs = {}, {}


def _model(L, dev):
    if L not in _models:
        m, sm = build_synth(C, G, H, L, seed=7300 + L, dev=dev)
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        dense = R.decode_volume(sm['coeffs'], sm['shape_array'], sm['filter_rev'])
        _models[L] = (m.eval(), sm, dense)
    return _models[L]


def _lattice_ref(L, res, dev):
    """The oracle on the reference's own tile positions, once per (net, lattice); never written to afterwards."""
    if (L, res) not in _refs:
        _m, sm, dense = _model(L, dev)
        rds = R.VolumeIndexing(res)
        ref = torch.empty(res)
        for b in R.tile_iter(rds.vol_res_touple, 32):
            yt = R.forward_from_grid(dense, sm['weights'], sm['biases'], R.tile_positions(rds, b).reshape(-1, 3), 2).clamp(-1, 1)
            ref[b[0]:b[1], b[2]:b[3], b[4]:b[5]] = yt.reshape(b[1] - b[0], b[3] - b[2], b[5] - b[4])
        _refs[(L, res)] = ref.numpy()
    return _refs[(L, res)]


def _both_wave_counts(run):
    """run(waves) under LFGC_FWD_WAVES=8 and =4 -> {8: result, 4: result}"""
    outs = {}
    for waves in (8, 4):
        os.environ['LFGC_FWD_WAVES'] = str(waves)
        try:
            outs[waves] = run(waves)
        finally:
            os.environ.pop('LFGC_FWD_WAVES', None)
    return outs


@pytest.mark.parametrize('sampler', ['zrun', 'gather'])
@pytest.mark.parametrize('res', LATTICES, ids=lambda r: 'x'.join(map(str, r)))
@pytest.mark.parametrize('L', LAYERS)
def test_lattice_bits_do_not_depend_on_waves_per_workgroup(dev, L, res, sampler):
    from latent_feature_grid_compression_amd import ops
    m, _sm, _dense = _model(L, dev)
    lattice = (res, 0, res[0], 32)

    def run(waves):
        with torch.no_grad():
            grid_cl = m._decoded_channel_last()
            plan = ops.forward_plan(m._descriptor(), grid_cl, lattice=lattice)
            assert (plan.CH, plan.MT, plan.resident, plan.waves, plan.x2) == (32, 4, 0, waves, 0)
            assert plan.zrun == int(sampler == 'zrun')
            if plan.zrun:
                tpr = (res[2] + 31) // 32
                assert plan.tiles_per_row == tpr and plan.ntiles == res[0] * res[1] * tpr
            y, _ = ops.forward_raw(m._descriptor(), grid_cl, m._packed(), lattice=lattice, clamp=True)
        torch.cuda.synchronize()
        return y.view(res).cpu()

    if sampler == 'gather':
        os.environ['LFGC_NO_ZRUN'] = '1'
    try:
        outs = _both_wave_counts(run)
    finally:
        os.environ.pop('LFGC_NO_ZRUN', None)
    ref = _lattice_ref(L, res, dev)
    for waves, y in outs.items():
        e = rel_err(y.numpy(), ref)
        print('MATE-PRIO lattice L%d %s %s waves %d | vs oracle %.3e' % (L, 'x'.join(map(str, res)), sampler, waves, e))
        assert e <= 1e-5, (waves, e)
    assert torch.equal(outs[8], outs[4]), 'output differs between 8- and 4-wave workgroups'


@pytest.mark.parametrize('L', LAYERS)
def test_position_list_and_stash_bits_do_not_depend_on_waves_per_workgroup(dev, L):
    from latent_feature_grid_compression_amd import ops
    m, sm, dense = _model(L, dev)
    rng = np.random.default_rng(7400 + L)
    pos = torch.from_numpy(rng.uniform(-1, 1, (N_POS, 3)).astype(np.float32))
    pos_d = pos.to(dev)

    def run(waves):
        with torch.no_grad():
            grid_cl = m._decoded_channel_last()
            plan = ops.forward_plan(m._descriptor(), grid_cl, pos=pos_d, want_stash=True)
            assert (plan.CH, plan.MT, plan.resident, plan.waves, plan.zrun) == (32, 4, 0, waves, 0)
            y, stash = ops.forward_raw(m._descriptor(), grid_cl, m._packed(), pos=pos_d, want_stash=True)
        torch.cuda.synchronize()
        return y.cpu(), _stash_live(stash, N_POS, plan, L).cpu()

    outs = _both_wave_counts(run)
    ref = R.forward_from_grid(dense, sm['weights'], sm['biases'], pos, 2).numpy()
    for waves, (y, _stash) in outs.items():
        e = rel_err(y.numpy(), ref)
        print('MATE-PRIO positions L%d n%d waves %d | vs oracle %.3e' % (L, N_POS, waves, e))
        assert e <= 1e-5, (waves, e)
    assert torch.equal(outs[8][0], outs[4][0]), 'output differs between 8- and 4-wave workgroups'
    assert torch.equal(outs[8][1], outs[4][1]), 'stash differs between 8- and 4-wave workgroups'
