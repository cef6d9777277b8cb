"""Record what the library's pure-host planners answer, as tests/golden/launch_plans.json.

    python tools/make_goldens_plans.py

Every field of lfgc_forward_plan (both launches), lfgc_backward_plan, lfgc_packed_bytes, lfgc_stash_bytes and
lfgc_backward_workspace_bytes over a table of network shapes, sample counts, lattices, precisions, stash and status
words.  Nothing is enqueued and no GPU is needed: without a device lfgc_num_cus() answers 256, the MI355X's count, and
the recorded plans are those of a 256-CU device.  The LFGC_* environment knobs are removed first.

The file is the yardstick of refactors of the planning code (tests/test_launch_plans_host.py compares field by field):
write it on the commit BEFORE the change and regenerate it after; the two must be the same bytes.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, '..'))
OUT = os.path.join(ROOT, 'tests', 'golden', 'launch_plans.json')

# (C, H, L): the three networks of BASELINE.json (2x32 on 16 channels, 4x64 on 16, 4x128 on 32), then the smallest net,
# odd channel counts, H = 96 (runs as 128) and the deepest net
SHAPES = [(16, 32, 2), (16, 64, 4), (32, 128, 4), (1, 16, 1), (9, 64, 3), (22, 96, 4), (24, 128, 8)]
N_SAMPLES = [0, 1, 255, 256, 257, 32768, 65536, 131072, 16777216]
# (res, x_begin, x_end, grid edge D = H = W)
LATTICES = [((32, 32, 32), 0, 32, 64), ((70, 40, 33), 0, 70, 64), ((256, 256, 256), 0, 256, 64),
            ((1024, 1024, 1024), 0, 16, 128)]
PRECISIONS = [0, 1, 2]
LAUNCH_FIELDS = ['resident', 'waves', 'coord_table', 'zrun', 'nzc', 'tiles_per_row', 'x2', 'lds_bytes', 'nbatches', 'ntiles',
                 'grid']
BACKWARD_FIELDS = ['CH', 'MT', 'waves', 'nslabs', 'roles', 'lds_bytes', 'nbatches', 'grid']


def clear_knobs(environ=os.environ):
    for k in [k for k in environ if k.startswith('LFGC_') and k != 'LFGC_LIB_PATH']:
        del environ[k]


def collect(lib, _lib):
    """The whole table as a JSON-able dict (lists of ints only)."""
    some_ptr = ctypes.c_void_p(16)            # `pos` is only tested against NULL
    sizes, forward, backward = [], [], []
    for si, (C, H, L) in enumerate(SHAPES):
        desc = _lib.MlpDesc(C, H, L, 2, 3, 1)
        counts = N_SAMPLES + [(xe - xb) * res[1] * res[2] for res, xb, xe, _ in LATTICES]
        sizes.append([si, lib.lfgc_packed_bytes(ctypes.byref(desc)),
                      [lib.lfgc_stash_bytes(ctypes.byref(desc), n) for n in counts],
                      [lib.lfgc_backward_workspace_bytes(ctypes.byref(desc), n) for n in counts]])
        positions = []
        for n in N_SAMPLES:
            positions.append((_lib.Positions(some_ptr, n, (ctypes.c_int32 * 3)(0, 0, 0), 0, 0, 0), 64))
        for res, xb, xe, D in LATTICES:
            positions.append((_lib.Positions(None, 0, (ctypes.c_int32 * 3)(*res), xb, xe, 32), D))
        for pi, (ps, D) in enumerate(positions):
            for prec in PRECISIONS:
                for stash in (0, 1):
                    for status in (0, 1):
                        info = _lib.ForwardPlanInfo()
                        rc = lib.lfgc_forward_plan(ctypes.byref(desc), ctypes.byref(ps), D, D, D, prec, stash, status,
                                                   ctypes.byref(info))
                        forward.append([si, pi, prec, stash, status, rc, info.CH, info.MT, info.has_redo, info.reserved] +
                                       [int(getattr(info.first, f)) for f in LAUNCH_FIELDS] +
                                       [int(getattr(info.redo, f)) for f in LAUNCH_FIELDS])
        for ni, n in enumerate(N_SAMPLES):
            for prec in PRECISIONS:
                info = _lib.BackwardPlanInfo()
                rc = lib.lfgc_backward_plan(ctypes.byref(desc), n, prec, ctypes.byref(info))
                backward.append([si, ni, prec, rc] + [int(getattr(info, f)) for f in BACKWARD_FIELDS])
    return {
        'num_cus': 256,
        'shapes_C_H_L': [list(s) for s in SHAPES],
        'n_samples': N_SAMPLES,
        'lattices_res_xbegin_xend_D': [[list(res), xb, xe, D] for res, xb, xe, D in LATTICES],
        'sizes_columns': ['shape', 'packed_bytes', 'stash_bytes per count', 'backward_workspace_bytes per count',
                          'counts = n_samples then the lattices\' sample counts'],
        'sizes': sizes,
        'forward_columns': ['shape', 'position (index into n_samples, then lattices)', 'precision', 'has_stash', 'has_status',
                            'rc', 'CH', 'MT', 'has_redo', 'reserved'] + ['first.' + f for f in LAUNCH_FIELDS] +
                           ['redo.' + f for f in LAUNCH_FIELDS],
        'forward': forward,
        'backward_columns': ['shape', 'n (index into n_samples)', 'precision', 'rc'] + BACKWARD_FIELDS,
        'backward': backward,
    }


def dumps(table) -> str:
    """One record per line: a changed field shows as one changed line."""
    lines = ['{']
    keys = list(table)
    for k in keys:
        v = table[k]
        tail = '' if k == keys[-1] else ','
        if k in ('sizes', 'forward', 'backward'):
            lines.append(' %s: [' % json.dumps(k))
            lines += ['  %s%s' % (json.dumps(r, separators=(',', ':')), '' if i == len(v) - 1 else ',') for i, r in enumerate(v)]
            lines.append(' ]' + tail)
        else:
            lines.append(' %s: %s%s' % (json.dumps(k), json.dumps(v), tail))
    lines.append('}')
    return '\n'.join(lines) + '\n'


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    clear_knobs()
    from latent_feature_grid_compression_amd import _lib
    text = dumps(collect(_lib.load(), _lib))
    with open(OUT, 'w') as f:
        f.write(text)
    print('wrote %s (%d bytes)' % (OUT, len(text)))
