"""Host tests of the empty-space skipping restatement (tests/skip_ref.py): hand-computed cases of the brick ranges, the
occupancy rule and the skip loop, and the share of skipped blocks in the scene the GPU test renders.  No GPU."""
import os
import re

import numpy as np

import render_ref as RR
import skip_ref as SR

F = np.float32


def test_brick_ranges_by_hand():
    vol = np.arange(5 * 3 * 3, dtype=F).reshape(5, 3, 3)                  # cells (4, 2, 2), B = 2: bricks (2, 1, 1)
    mm = SR.brick_minmax(vol, 2)
    assert mm.shape == (2, 1, 1, 2)
    assert mm[0, 0, 0].tolist() == [0.0, 26.0]                            # planes 0..2: the face plane 2 belongs to both
    assert mm[1, 0, 0].tolist() == [18.0, 44.0]                           # planes 2..4
    vol[2, 1, 1] = np.nan                                                 # on the shared face
    mm = SR.brick_minmax(vol, 2)
    assert mm[0, 0, 0].tolist() == [-np.inf, np.inf] and mm[1, 0, 0].tolist() == [-np.inf, np.inf]
    one = SR.brick_minmax(np.array([[[1.0, 2.0], [3.0, 4.0]], [[-5.0, 6.0], [7.0, 8.0]]], F), 8)      # 2 x 2 x 2, one cell
    assert one.shape == (1, 1, 1, 2) and one[0, 0, 0].tolist() == [-5.0, 8.0]
    assert SR.brick_counts((9, 8, 16), 8) == (2, 1, 2)                    # a one-cell last brick


def test_the_guard_is_the_headers_number():
    """LFGC_RAY_SKIP_GUARD of include/lfgc.h (lfgc_ray_skip_f32's) is Render.touched_bricks' guard and the restatement's."""
    from latent_feature_grid_compression_amd.visualization import Render
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(os.path.dirname(__file__), '..', 'include', 'lfgc.h')).read(), flags=re.S)
    m = re.findall(r'^[ \t]*#[ \t]*define[ \t]+LFGC_RAY_SKIP_GUARD[ \t]+([0-9.eE+-]+)f[ \t]*$', header, flags=re.M)
    assert len(m) == 1, 'LFGC_RAY_SKIP_GUARD is not defined exactly once in include/lfgc.h'
    assert float(F(m[0])) == float(m[0]) > 0.0                            # the literal is an fp32 number
    assert Render._SKIP_GUARD == float(m[0]) and SR.GUARD.dtype == F and SR.GUARD == F(m[0])


def _occ(ranges, ext, margin, v_min=-1.0, v_max=1.0):
    table = np.zeros((len(ext), 4), F)
    table[:, 3] = ext
    return SR.occupancy(np.array(ranges, F), table, v_min, v_max, margin).tolist()


def test_occupancy_by_hand():
    inf = np.inf
    # two rows: nodes at -1 and 1
    assert _occ([(-1, -1), (-1, -0.5), (-3, -2), (1, 1), (2, 3)], [0, 5], 0.0) == [0, 1, 0, 1, 1]
    assert _occ([(-1, -1), (1, 1), (2, 3), (0.99, 3), (-inf, inf)], [5, 0], 0.0) == [1, 0, 0, 1, 1]
    # five rows: nodes at -1, -0.5, 0, 0.5, 1; transparent up to the node 0
    ext = [0, 0, 0, 4, 8]
    assert _occ([(-1, 0), (0, 0), (-0.5, 1e-3), (0.5, 0.5), (-7, -0.25), (-inf, inf), (-inf, 0)], ext, 0.0) == [0, 0, 1, 1, 0, 1, 0]
    assert _occ([(-1, 0), (-1, -1e-4), (-1, -1e-5)], ext, 1e-5) == [1, 0, 0]        # a margin that just reaches row 3
    # transparent between two opaque ends: the range may touch the nodes -0.5 and 0.5 but not pass them
    ext = [3, 0, 0, 0, 2]
    assert _occ([(-0.5, 0.5), (-0.5, 0.5)], ext, 0.0) == [0, 0]
    assert _occ([(-0.5, 0.5), (-0.51, 0), (0, 0.51), (2, 2), (-2, -2)], ext, 1e-5) == [1, 1, 1, 1, 1]
    # an all-zero table sees nothing anywhere
    assert _occ([(-1, 1), (-inf, inf), (5, 6)], [0, 0, 0], 0.0) == [0, 0, 0]


def test_skip_of_an_axis_parallel_ray_by_hand():
    """Box +-1, 32 cells per axis, B = 4: eight bricks of width 0.25 per axis.  Rays along +x from x = -3 with dt = 1/64:
    128 steps, sample k at x = -1 + (k + 0.5)/64, i.e. cell coordinate (k + 0.5)/4 -- at least 1/8 cell from a cell face,
    so the guard of 1/16 never reaches a neighbour.  A block of 32 steps covers the x bricks 2b and 2b + 1.  y = z = 0.1
    is the cell coordinate 17.6: brick 4."""
    box = ([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0])
    cells, B, S, dt = (32, 32, 32), 4, 32, 1.0 / 64.0
    o = np.array([[-3.0, 0.1, 0.1], [-3.0, 0.6, 0.1], [-3.0, 0.1, 0.1], [-3.0, 0.1, 0.1]], F)
    d = np.array([[1.0, 0.0, 0.0]] * 4, F)
    tn, tf, n = RR.clip(o, d, box[0], box[1], 0.0, np.inf, dt, 1000)
    assert n.tolist() == [128] * 4 and tn.tolist() == [2.0] * 4
    occ = np.zeros((8, 8, 8), np.uint8)
    occ[5, 4, 4] = 1                                                      # x in [0.25, 0.5]: steps 80 .. 95, block 2
    k0 = np.array([0, 0, 96, 64], np.int32)
    k, s = SR.skip([0, 1, 2, 3], o, d, tn, tf, n, k0, dt, S, box[0], box[1], cells, B, occ)
    # ray 0 jumps the blocks 0 and 1 and stops in front of block 2; ray 1 (y brick 6) never meets the brick; ray 2 starts
    # behind it and runs out; ray 3 starts at the block that holds it and does not move
    assert k.tolist() == [64, 128, 128, 64] and s.tolist() == [2, 4, 1, 0]
    # S = 64: the blocks hold the x bricks 0..3 and 4..7
    k, s = SR.skip([0, 1], o, d, tn, tf, n, np.zeros(4, np.int32), dt, 64, box[0], box[1], cells, B, occ)
    assert k.tolist() == [64, 128, 0, 0] and s.tolist() == [1, 2, 0, 0]
    # all occupied: nothing moves; all empty: every ray ends past its last step
    k, s = SR.skip([0, 1, 2, 3], o, d, tn, tf, n, k0, dt, S, box[0], box[1], cells, B, np.ones((8, 8, 8), np.uint8))
    assert k.tolist() == k0.tolist() and s.tolist() == [0, 0, 0, 0]
    k, s = SR.skip([0, 1, 2, 3], o, d, tn, tf, n, k0, dt, S, box[0], box[1], cells, B, np.zeros((8, 8, 8), np.uint8))
    assert k.tolist() == [128] * 4 and s.tolist() == [4, 4, 1, 2]


def test_the_gpu_scene_has_empty_and_occupied_space():
    """The ground-truth scene of tests/test_render_skip_gpu.py by the restatement alone: at least a quarter of the blocks
    are skipped and at least a twentieth are evaluated, so that test exercises both."""
    scales = [float(s) for s in SR.scene_scales()]
    box = ([-s for s in scales], scales)
    vol = SR.scene_volume()
    cells = [r - 1 for r in SR.SCENE_RES]
    occ = SR.occupancy(SR.brick_minmax(vol, SR.SCENE_BRICK), SR.scene_table(), -1.0, 1.0, 1e-5)
    assert occ.shape == (10, 9, 8) and 0.02 < occ.mean() < 0.5
    o, d = SR.scene_rays()
    o, d = o.numpy(), (d / d.norm(dim=1, keepdim=True)).numpy()
    from latent_feature_grid_compression_amd.visualization.Render import max_steps_for
    tn, tf, n = RR.clip(o, d, box[0], box[1], 0.0, np.inf, SR.SCENE_STEP, max_steps_for(box[0], box[1], SR.SCENE_STEP))
    blocks, skipped, evaluated = SR.march(o, d, tn, tf, n, SR.SCENE_STEP, 32, box[0], box[1], cells, SR.SCENE_BRICK, occ)
    print('scene: %d rays hit, %d blocks, %d skipped, %d evaluated, %.1f %% of %s bricks occupied'
          % ((n > 0).sum(), blocks, skipped, evaluated, 100.0 * occ.mean(), occ.shape))
    assert skipped + evaluated == blocks
    assert skipped >= blocks / 4 and evaluated >= blocks / 20
