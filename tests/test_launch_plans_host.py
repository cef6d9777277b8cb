"""CPU test: the library's pure-host planners -- lfgc_forward_plan (both launches), lfgc_backward_plan,
lfgc_packed_bytes, lfgc_stash_bytes, lfgc_backward_workspace_bytes -- answer what tests/golden/launch_plans.json
records (tools/make_goldens_plans.py), field for field.  The file was written by the commit before the kernels and
planners began to take their shapes and LDS sizes from the one constexpr plan of csrc/lfgc_common.h; a planner that
drifts from it sizes an LDS allocation its kernel does not carve.

Without a device lfgc_num_cus() answers 256, the MI355X's count, which is what the file holds."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'launch_plans.json')


def _tool():
    spec = importlib.util.spec_from_file_location('make_goldens_plans', os.path.join(ROOT, 'tools', 'make_goldens_plans.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _other_cu_count():
    """CU count of a present device if it is not the 256 the fixture was recorded for, else None."""
    import torch
    if not torch.cuda.is_available():
        return None
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return None if cus == 256 else cus


def test_launch_plans_match_the_recorded_ones(monkeypatch):
    cus = _other_cu_count()
    if cus is not None:
        pytest.skip('launch_plans.json holds the plans of a 256-CU device; this one has %d' % cus)
    tool = _tool()
    for k in [k for k in os.environ if k.startswith('LFGC_') and k != 'LFGC_LIB_PATH']:
        monkeypatch.delenv(k)
    from latent_feature_grid_compression_amd import _lib
    got = tool.collect(_lib.load(), _lib)
    want = json.load(open(GOLD))
    assert list(got) == list(want)
    for key in want:
        if key not in ('sizes', 'forward', 'backward'):
            assert got[key] == want[key], key
    assert want['num_cus'] == 256
    # every record, and inside a record every field, by name
    columns = {'forward': want['forward_columns'], 'backward': want['backward_columns']}
    wrong = []
    for key in ('forward', 'backward'):
        assert len(got[key]) == len(want[key])
        for g, w in zip(got[key], want[key]):
            assert len(g) == len(w) == len(columns[key])
            wrong += ['%s %s: %s = %d, recorded %d' % (key, w[:5], columns[key][i], g[i], w[i])
                      for i in range(len(w)) if g[i] != w[i]]
    assert len(got['sizes']) == len(want['sizes'])
    for g, w in zip(got['sizes'], want['sizes']):
        shape = want['shapes_C_H_L'][w[0]]
        if g[:2] != w[:2]:
            wrong.append('sizes %s: packed_bytes = %d, recorded %d' % (shape, g[1], w[1]))
        for name, gs, ws in (('stash_bytes', g[2], w[2]), ('backward_workspace_bytes', g[3], w[3])):
            assert len(gs) == len(ws)
            wrong += ['sizes %s: %s[count %d] = %d, recorded %d' % (shape, name, i, gs[i], ws[i])
                      for i in range(len(ws)) if gs[i] != ws[i]]
    assert not wrong, '%d fields differ:\n%s' % (len(wrong), '\n'.join(wrong[:40]))
    # and the file itself is what the tool writes
    assert tool.dumps(got) == open(GOLD).read()


def test_the_table_reaches_every_kind_of_launch():
    """The recorded cases are worth comparing against: resident and streamed nets, 4- and 8-wave workgroups, coordinate
    tables, z-run launches, the range fallback, and the slab split of the weight-gradient kernel all occur."""
    t = json.load(open(GOLD))
    fc, bc = t['forward_columns'], t['backward_columns']
    col = lambda rows, cols, name: {r[cols.index(name)] for r in rows}
    assert col(t['forward'], fc, 'rc') == {0} and col(t['backward'], bc, 'rc') == {0}
    assert col(t['forward'], fc, 'first.resident') == {0, 1}
    assert col(t['forward'], fc, 'first.waves') == {4, 8} and col(t['backward'], bc, 'waves') == {4, 8}
    assert col(t['forward'], fc, 'first.coord_table') == {0, 1}
    assert col(t['forward'], fc, 'first.zrun') == {0, 1}
    assert col(t['forward'], fc, 'has_redo') == {0, 1}
    assert col(t['forward'], fc, 'CH') == {8, 16, 24, 32} and col(t['forward'], fc, 'MT') == {1, 2, 4}
    assert len(col(t['backward'], bc, 'roles')) > 1
    assert os.path.getsize(GOLD) < 256 * 1024
