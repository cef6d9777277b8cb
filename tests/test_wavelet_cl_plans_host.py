"""CPU test of the launch-plan queries of the channel-last last level (lfgc_idwt_level_cl_plan, lfgc_idwt_level_cl_bwd_plan;
csrc/lfgc_wavelet_cl.hip) with an explicit CU count, i.e. pure host arithmetic: the selection functions that fill the
queried struct are the ones the launchers consume, so what is pinned here is what is launched.  The rules are restated
here and in tests/wavelet_bound.py (cl_expected_plan, cl_pick_zchunk) from the source comments and DESIGN section 3.2.1,
not read back from the library: channel-group width, adjoint cell groups, streaming stores, both LDS formulas, the z
chunking per CU count, each diagnostics knob, the error codes, and the slice count ops._adjoint sizes its
deterministic-mode scratch with.

Also pins the componentwise checker (tests/wavelet_bound.py) on this kernel family's characteristic fault, in numpy: a z
chunk that starts without its warm-up planes.  Measured here (d = (6,4,5), chunks of 3 cell slices, db2 and a 6-tap
bank): the restatement lands at 1.9 to 3.1 units of 2^-24 * mag, the seam fault at 1.6e7 units at every scale, and
max|err| / max|ref| falls from 0.6 - 0.8 to 1.1e-7 once the planes the seam slices are made of are scaled to 1e-7."""
import ctypes
import os

import numpy as np
import pytest
import torch

import wavelet_bound as W

OK, E_NULL, E_SHAPE, E_UNSUPPORTED = 0, -1, -2, -3
CUS = (256, 64, 32, 8)
FIELDS = ('cw', 'cells', 'nt', 'drop', 'zchunk', 'nchunks', 'ptiles', 'ngroups', 'threads', 'lds_bytes', 'blocks')
ENTRY = {False: 'lfgc_idwt_level_cl_plan', True: 'lfgc_idwt_level_cl_bwd_plan'}


@pytest.fixture(scope='module')
def lib():
    from latent_feature_grid_compression_amd import _lib
    return _lib.load()


class knobs:
    """The diagnostics switches of the channel-last level for the duration of a block (kw: cw, nt, ng, nchunks)."""

    def __init__(self, **kv):
        self.kv = {W.CL_KNOBS[k]: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        for k, v in self.kv.items():
            assert k not in os.environ, k
            os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k in self.kv:
            os.environ.pop(k, None)


def query(lib, adjoint, L, drop, C, d, t, num_cus, cs=None):
    """(return code, dict of the struct's fields) of a plan entry."""
    from latent_feature_grid_compression_amd import _lib
    info = _lib.WaveletClPlanInfo()
    rc = getattr(lib, ENTRY[adjoint])(L, int(drop), C, (C + 7) // 8 * 8 if cs is None else cs, *d, *t, num_cus, ctypes.byref(info))
    p = {k: int(getattr(info, k)) for k in FIELDS}
    p['nt'], p['drop'] = bool(p['nt']), bool(p['drop'])
    return rc, p


def plan(lib, adjoint, L, drop, C, d, t, num_cus):
    rc, p = query(lib, adjoint, L, drop, C, d, t, num_cus)
    assert rc == OK, (adjoint, L, drop, C, d, t, num_cus, rc)
    return p


def full(d, L):
    return tuple(2 * v + L - 2 for v in d)


def invariants(p, nz):
    assert p['lds_bytes'] <= W.CL_LDS_CAP
    assert p['blocks'] % 8 == 0 and 0 <= p['blocks'] - p['ptiles'] * p['ngroups'] * p['nchunks'] < 8
    assert p['nchunks'] * p['zchunk'] >= nz and (p['nchunks'] - 1) * p['zchunk'] < nz       # no empty chunk
    assert p['threads'] == 32 * p['cw'] <= 1024


# ---- channel-group width, cell groups, streaming stores -----------------------------------------------------------------

@pytest.mark.parametrize('L', [2, 4])
def test_synthesis_channel_width(lib, L):
    K = L // 2
    # stride 32, ptiles = ceil((d1 + K - 1)(d2 + K - 1) / 32) of 95 and 96: Haar planes of 3040 and 3041 cells, db2 planes
    # of 1520 x 2 = 3040 and 1521 x 2 = 3042 cells
    for d, ptiles, cw in (((3, 3040, 1), 95, 16), ((3, 3041, 1), 96, 32)) if K == 1 else (((3, 1519, 1), 95, 16), ((3, 1520, 1), 96, 32)):
        assert -(-(d[1] + K - 1) * (d[2] + K - 1) // 32) == ptiles
        for drop in (False, True):
            for C in (25, 32):
                p = plan(lib, False, L, drop, C, d, full(d, L), 256)
                assert (p['cw'], p['ngroups'], p['ptiles'], p['cells']) == (cw, 32 // cw, ptiles, 32), p
    d = (3, 60, 60)                                     # a large plane does not widen the other strides
    for C, cw, ngroups in ((16, 16, 1), (9, 16, 1), (8, 8, 1), (1, 8, 1), (24, 8, 3), (17, 8, 3), (40, 8, 5), (48, 8, 6)):
        p = plan(lib, False, L, False, C, d, full(d, L), 256)
        assert (p['cw'], p['ngroups']) == (cw, ngroups), (C, p)


@pytest.mark.parametrize('L', [2, 4])
def test_adjoint_channel_width_and_cell_groups(lib, L):
    for C, cw, ngroups in ((32, 16, 2), (25, 16, 2), (16, 16, 1), (8, 8, 1), (24, 8, 3), (40, 8, 5), (48, 16, 3)):
        for d, ng in (((2, 37, 83), 1), ((2, 48, 64), 2), ((2, 1, 3071), 1), ((2, 3072, 1), 2)):     # d1 d2 = 3071 / 3072
            assert (d[1] * d[2] >= 3072) == (ng == 2)
            for drop in (False, True):
                if C > 32 and drop:
                    continue
                p = plan(lib, True, L, drop, C, d, full(d, L), 256)
                assert (p['cw'], p['ngroups'], p['cells'], p['ptiles']) == (cw, ngroups, 32 * ng, -(-d[1] * d[2] // (32 * ng))), p
                assert p['nt'] is False and p['drop'] is drop


def test_streaming_stores_above_48_mib_of_grid(lib):
    """Arithmetic only: t0 t1 t2 * 32 channels * 4 bytes against 48 MiB = 393 216 voxels, both sides; only for CW = 32."""
    d = (49, 64, 64)
    for t, nt in (((96, 64, 64), False), ((96, 64, 64 + 1), True), ((97, 64, 64), True)):
        assert (t[0] * t[1] * t[2] * 32 * 4 > 48 << 20) == nt
        for L in (2, 4):
            for drop in (False, True):
                p = plan(lib, False, L, drop, 32, d, t, 256)
                assert p['cw'] == 32 and p['nt'] is nt, (t, p)
    # the same voxels in 16 channels (twice the extent): 16-channel workgroups never stream
    p = plan(lib, False, 4, False, 16, (48, 64, 128), (97, 64, 129), 256)
    assert p['cw'] == 16 and p['nt'] is False
    # stride 32 on a small plane (CW = 16) does not stream however large the grid
    d, t = (500, 30, 30), (1000, 60, 60)
    assert t[0] * t[1] * t[2] * 32 * 4 > 48 << 20
    p = plan(lib, False, 4, False, 32, d, t, 256)
    assert p['cw'] == 16 and p['nt'] is False


def test_lds_formulas(lib):
    """Synthesis: two tiles [8 parities][32 cells][CW + 1] (+ DROP: two factor tables [K^2][8][32]); adjoint: two tiles
    [CW][8 * cells + 1]."""
    seen = set()
    for L in (2, 4):
        K = L // 2
        for C, d in ((32, (2, 56, 56)), (32, (2, 9, 9)), (16, (2, 9, 9)), (8, (2, 9, 9)), (24, (2, 56, 56)), (16, (2, 56, 56))):
            for drop in (False, True):
                p = plan(lib, False, L, drop, C, d, full(d, L), 256)
                assert p['lds_bytes'] == 2 * 8 * 32 * (p['cw'] + 1) * 4 + (2 * 8 * K * K * 32 * 4 if drop else 0)
                b = plan(lib, True, L, drop, C, d, full(d, L), 256)
                assert b['lds_bytes'] == 2 * b['cw'] * (8 * b['cells'] + 1) * 4
                assert max(p['lds_bytes'], b['lds_bytes']) <= W.CL_LDS_CAP
                seen |= {('fwd', p['cw']), ('bwd', b['cw'], b['cells'])}
    assert seen == {('fwd', 8), ('fwd', 16), ('fwd', 32), ('bwd', 8, 32), ('bwd', 8, 64), ('bwd', 16, 32), ('bwd', 16, 64)}
    # the largest of each: 67 584 + 8192 and 65 664 bytes
    assert plan(lib, False, 4, True, 32, (2, 56, 56), (6, 114, 114), 256)['lds_bytes'] == 75776
    assert plan(lib, True, 4, True, 32, (2, 56, 56), (6, 114, 114), 256)['lds_bytes'] == 65664


# ---- z chunking ---------------------------------------------------------------------------------------------------------

def test_restated_chunk_rule_on_known_points():
    """The restatement itself, by hand: one column of 7 steps on one slot takes the whole walk (cost 1 * 8; 7 chunks of one
    step would cost 7 * 2); with 7 slots free, 7 chunks of 1 (cost 1 * 2)."""
    assert W.cl_pick_zchunk(1, 7, 1, 1) == 7
    assert W.cl_pick_zchunk(1, 7, 1, 7) == 1
    assert W.cl_pick_zchunk(1, 7, 1, 4) == 2          # 4 chunks of 2: 1 * 3; 2 of 4: 1 * 5; 7 of 1: 2 * 2
    assert [W.cl_pick_zchunk(1, 7, 1, 1, n) for n in (1, 2, 3, 7, 0, 8)] == [7, 4, 3, 1, 7, 7]


@pytest.mark.parametrize('num_cus', CUS)
@pytest.mark.parametrize('L', [2, 4])
def test_zchunk_is_the_cost_rule(lib, L, num_cus):
    K = L // 2
    shapes = ((5, (7, 9)), (13, (12, 7)), (30, (9, 12)), (32, (56, 56)), (22, (35, 6)), (8, (56, 56)), (32, (64, 64)))
    for d0 in range(1, 41):
        for C, plane in shapes:
            d = (d0,) + plane
            t = full(d, L)
            for adjoint in (False, True):
                for drop in (False, True):
                    p = plan(lib, adjoint, L, drop, C, d, t, num_cus)
                    want = W.cl_expected_plan(adjoint, L, C, d, t, drop, num_cus)
                    assert p == want, (adjoint, drop, C, d, p, want)
                    invariants(p, d0 if adjoint else d0 + K - 1)


def test_zchunk_depends_on_the_cu_count_and_on_the_drop_slots(lib):
    """Why the query takes the count: the same shape chunks differently on another partition, and the DROP build of the
    db2 adjoint with 32-cell tiles (2 instead of 3, 5 instead of 6 workgroups per CU) chunks differently from the plain one."""
    d, t = (33, 33, 33), (64, 64, 64)
    assert len({plan(lib, False, 4, False, 32, d, t, n)['zchunk'] for n in CUS}) > 1
    assert len({plan(lib, True, 4, False, 32, d, t, n)['zchunk'] for n in CUS}) > 1
    differs = 0
    for C, dd in ((13, (5, 12, 7)), (5, (6, 7, 9)), (22, (4, 35, 6)), (30, (5, 9, 12)), (32, (33, 33, 33)), (8, (33, 33, 33))):
        for n in CUS:
            a, b = (plan(lib, True, 4, drop, C, dd, full(dd, 4), n) for drop in (False, True))
            assert a == dict(W.cl_expected_plan(True, 4, C, dd, full(dd, 4), False, n))
            assert b == dict(W.cl_expected_plan(True, 4, C, dd, full(dd, 4), True, n))
            differs += a['zchunk'] != b['zchunk']
            h0, h1 = (plan(lib, True, 2, drop, C, dd, full(dd, 2), n) for drop in (False, True))
            assert {k: v for k, v in h0.items() if k != 'drop'} == {k: v for k, v in h1.items() if k != 'drop'}   # Haar: same slots
    assert differs > 0


def test_num_cus_zero_is_the_current_device(lib):
    """Without a device the library's CU count is 256, the MI355X's (tests/test_launch_plans_host.py); with one, its own."""
    n = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    for C, d in ((32, (33, 33, 33)), (13, (5, 12, 7))):
        for adjoint in (False, True):
            assert plan(lib, adjoint, 4, False, C, d, full(d, 4), 0) == plan(lib, adjoint, 4, False, C, d, full(d, 4), n)


# ---- the diagnostics knobs ----------------------------------------------------------------------------------------------

def _both(lib, L, C, d, num_cus=64):
    t = W.cl_target(L, d)
    return {(adj, drop): plan(lib, adj, L, drop, C, d, t, num_cus) for adj in (False, True) for drop in (False, True)}


@pytest.mark.parametrize('L', [2, 4])
def test_knobs_change_the_field_they_name(lib, L):
    C, d = 30, (5, 9, 12)
    t = W.cl_target(L, d)
    base = _both(lib, L, C, d)
    assert base[(False, False)]['cw'] == 16 and base[(True, False)]['cells'] == 32
    shape = ('cw', 'cells', 'nt', 'drop')
    for cw in (8, 16, 32):
        with knobs(cw=cw):
            got = _both(lib, L, C, d)
        for key, p in got.items():
            adjoint, drop = key
            assert p == W.cl_expected_plan(adjoint, L, C, d, t, drop, 64, cw=cw), (cw, key)
            if adjoint:
                assert p == base[key]                              # the adjoint has no such switch
            else:
                assert p['cw'] == cw and p['ngroups'] == 32 // cw and p['threads'] == 32 * cw
                assert [p[k] for k in shape[1:]] == [base[key][k] for k in shape[1:]] and p['ptiles'] == base[key]['ptiles']
    for nt in (0, 1):
        with knobs(nt=nt):
            got = _both(lib, L, C, d)
        for key, p in got.items():
            assert p == dict(base[key], nt=(bool(nt) and not key[0])), (nt, key)
    for ng in (1, 2):
        with knobs(ng=ng):
            got = _both(lib, L, C, d)
        for key, p in got.items():
            adjoint, drop = key
            assert p == W.cl_expected_plan(adjoint, L, C, d, t, drop, 64, ng=ng), (ng, key)
            if not adjoint:
                assert p == base[key]
            else:
                assert p['cells'] == 32 * ng and p['ptiles'] == -(-108 // (32 * ng))
                assert [p[k] for k in ('cw', 'nt', 'drop', 'ngroups', 'threads')] == [base[key][k] for k in ('cw', 'nt', 'drop', 'ngroups', 'threads')]
    for n in (1, 2, 3, 5):
        with knobs(nchunks=n):
            got = _both(lib, L, C, d)
        for key, p in got.items():
            nz = d[0] if key[0] else d[0] + L // 2 - 1
            assert p['zchunk'] == -(-nz // n) and p['nchunks'] == -(-nz // p['zchunk'])
            rest = lambda q: {k: v for k, v in q.items() if k not in ('zchunk', 'nchunks', 'blocks')}
            assert rest(p) == rest(base[key])
            invariants(p, nz)
    # a width that is not a channel-group size or does not divide the stride, a third cell group, a chunk count outside
    # 1..nz: ignored, nothing changes
    for kv in ({'cw': 12}, {'cw': 64}, {'cw': 0}, {'ng': 3}, {'ng': 0}, {'nchunks': 0}, {'nchunks': -1}, {'nchunks': 7}):
        with knobs(**kv):
            assert _both(lib, L, C, d) == base, kv
    base24 = _both(lib, L, 22, (4, 35, 6))
    for kv in ({'cw': 16}, {'cw': 32}):                              # stride 24
        with knobs(**kv):
            assert _both(lib, L, 22, (4, 35, 6)) == base24, kv
    assert not any(k in os.environ for k in W.CL_KNOBS.values())


# ---- the GPU cases ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,C,d,kn,cw,acw,ng', W.CL_ROWS, ids=[r[0] for r in W.CL_ROWS])
def test_gpu_rows_reach_the_named_paths(lib, name, C, d, kn, cw, acw, ng):
    for L in (2, 4):
        t = W.cl_target(L, d)
        K = L // 2
        assert all(1 <= tv <= 2 * dv + L - 2 for tv, dv in zip(t, d))
        assert (L == 2 and t == tuple(2 * v for v in d)) or (L == 4 and sorted(2 * dv + 2 - tv for tv, dv in zip(t, d)) == [0, 0, 1])
        for n in CUS:
            for drop in (False, True):
                with knobs(**kn):
                    f, b = plan(lib, False, L, drop, C, d, t, n), plan(lib, True, L, drop, C, d, t, n)
                assert f == W.cl_expected_plan(False, L, C, d, t, drop, n, **kn) and f['cw'] == cw and not f['nt'], (name, f)
                assert b == W.cl_expected_plan(True, L, C, d, t, drop, n, **kn) and (b['cw'], b['cells']) == (acw, 32 * ng), (name, b)
                invariants(f, d[0] + K - 1)
                invariants(b, d[0])
    if name == 'cw32_ng2':
        assert [plan(lib, False, L, False, C, d, W.cl_target(L, d), 256)['ptiles'] for L in (4, 2)] == [102, 98]
    if name.startswith('adj_ng2_forced_ragged'):
        assert d[1] * d[2] == 108 and b['ptiles'] == 2               # tile 1: cells 64..107, its second group has 12 of 32
    if name == 'adj_ng2_forced_empty_group':
        assert d[1] * d[2] == 70 and b['ptiles'] == 2                # tile 1: cells 64..69, its second group has none


def test_gpu_rows_cover_every_instantiation_family():
    """Synthesis K x CW {8,16,32} x DROP, adjoint K x CW {8,16} x NG {1,2} x DROP: every row runs both bases, plain and
    DROP; the streaming-store builds run on one row per CW."""
    assert {r[4] for r in W.CL_ROWS} == {8, 16, 32}
    assert {(r[5], r[6]) for r in W.CL_ROWS} == {(8, 1), (8, 2), (16, 1), (16, 2)}
    assert {c for c, _ in ((W.cl_expected_plan(False, 4, C, d, W.cl_target(4, d), False, 256, **kn)['cw'], n)
                           for n, C, d, kn, *_ in (W.CL_ROW[k] for k in ('cw8_one_group', 'cw16_stride16', 'cw32_forced_small_plane')))} == {8, 16, 32}


@pytest.mark.parametrize('L', [2, 4])
def test_forced_chunkings_of_seven_steps(lib, L):
    for _name, C, plane in W.CL_CHUNK_ROWS:
        for adjoint in (False, True):
            d = W.cl_chunk_shape(L, plane, adjoint)
            assert (d[0] if adjoint else d[0] + L // 2 - 1) == 7
            for n, lengths in zip(W.CL_NCHUNKS, ((7,), (4, 3), (3, 3, 1), (1,) * 7)):
                with knobs(nchunks=n):
                    p = plan(lib, adjoint, L, False, C, d, W.cl_target(L, d), 256)
                assert (p['zchunk'], p['nchunks']) == (lengths[0], len(lengths))
                assert tuple(min(p['zchunk'], 7 - i * p['zchunk']) for i in range(p['nchunks'])) == lengths


def test_reference_magnitudes_are_positive_for_the_gpu_rows():
    """No element of any tensor of any case is outside the componentwise bound (W.cl_case asserts mag > 0 for each)."""
    for name, C, d, *_ in W.CL_ROWS:
        if C * d[1] * d[2] > 20000:
            continue                                                 # the 56 x 56 planes: asserted when the GPU test builds them
        for L in (2, 4):
            for variant in ('plain', 'drop') + (('masked',) if name in W.CL_MASKED_ROWS else ()):
                case = W.cl_case(L, C, d, variant)
                assert set(case.ref) == ({'out', 'd_lll', 'd_hf'} | ({'d_ml', 'd_mh'} if variant != 'plain' else set()))
                assert min(float(m.min()) for _r, m in case.ref.values()) > 0


# ---- error codes --------------------------------------------------------------------------------------------------------

def test_plan_queries_report_the_launch_codes(lib):
    d, t = (3, 3, 3), (6, 6, 6)
    for adjoint in (False, True):
        entry = getattr(lib, ENTRY[adjoint])
        assert entry(4, 0, 8, 8, *d, *t, 256, None) == E_NULL
        for L in (0, 1, 3, 6, 8):
            assert query(lib, adjoint, L, False, 8, d, t, 256)[0] == E_UNSUPPORTED
        for C, cs in ((5, 5), (5, 16), (8, 16), (9, 8), (32, 40)):     # not roundup(C, 8)
            assert query(lib, adjoint, 4, False, C, d, t, 256, cs=cs)[0] == E_SHAPE
        assert query(lib, adjoint, 4, False, 8, d, (9, 6, 6), 256)[0] == E_SHAPE       # t > 2 d + L - 2
        assert query(lib, adjoint, 4, False, 8, d, (8, 8, 8), 256)[0] == OK
        assert query(lib, adjoint, 2, False, 8, d, (7, 6, 6), 256)[0] == E_SHAPE
        assert query(lib, adjoint, 4, False, 0, d, t, 256, cs=8)[0] == E_SHAPE
        assert query(lib, adjoint, 4, False, 8, (3, 0, 3), t, 256)[0] == E_SHAPE
        # arrays of 2^30 bytes: the grid (t0 t1 t2 * stride * 4) and the detail coefficients (7 C d0 d1 d2 * 4)
        assert query(lib, adjoint, 4, False, 32, (128, 128, 64), (256, 256, 128), 256)[0] == E_UNSUPPORTED
        assert query(lib, adjoint, 4, False, 32, (128, 128, 64), (256, 256, 127), 256)[0] == OK
        assert query(lib, adjoint, 4, False, 32, (128, 128, 73), (1, 1, 1), 256)[0] == OK            # 7 * 32 * 2^14 * 73 * 4 < 2^30
        assert query(lib, adjoint, 4, False, 32, (128, 128, 74), (1, 1, 1), 256)[0] == E_UNSUPPORTED
        # C > 32: the plain pair takes it, the drop pair does not
        assert query(lib, adjoint, 4, False, 40, d, t, 256)[0] == OK
        assert query(lib, adjoint, 4, True, 40, d, t, 256)[0] == E_UNSUPPORTED
    # the launch agrees where it decides on the host: NULL pointers first, then the same codes
    one = ctypes.c_void_p(16)                                      # any non-NULL address: nothing is launched on these paths
    taps = (ctypes.c_float * 8)(*[0.5] * 8)
    assert lib.lfgc_idwt_level_cl_len_f32(one, one, taps, 6, one, 8, 8, *d, *t, None) == E_UNSUPPORTED
    assert lib.lfgc_idwt_level_cl_len_f32(one, one, taps, 4, one, 5, 16, *d, *t, None) == E_SHAPE
    assert lib.lfgc_idwt_level_cl_bwd_len_f32(one, taps, 4, one, one, 8, 8, *d, 9, 6, 6, None) == E_SHAPE
    assert lib.lfgc_idwt_level_cl_bwd_len_f32(one, taps, 4, one, one, 32, 32, 128, 128, 74, 1, 1, 1, None) == E_UNSUPPORTED
    assert lib.lfgc_idwt_level_cl_len_f32(None, one, taps, 4, one, 8, 8, *d, *t, None) == E_NULL
    nan = float('nan')
    assert lib.lfgc_idwt_level_cl_drop_len_f32(one, one, one, nan, one, nan, taps, 4, one, 40, 40, *d, *t, None) == E_UNSUPPORTED


def test_wrappers_return_the_struct(lib):
    from latent_feature_grid_compression_amd import ops
    d = (5, 9, 12)
    for L in (2, 4):
        t = W.cl_target(L, d)
        for drop in (False, True):
            assert vars(ops.idwt_level_cl_plan(L, 30, d, t, has_drop=drop, num_cus=32)) == plan(lib, False, L, drop, 30, d, t, 32)
            assert vars(ops.idwt_level_cl_bwd_plan(L, 30, d, t, has_drop=drop, num_cus=32)) == plan(lib, True, L, drop, 30, d, t, 32)


def test_adjoint_slice_count_is_the_plans_group_count(lib):
    """ops._adjoint sizes the deterministic mode's scratch with one slice per channel group of the launch: it asks the
    selection, and the selection runs groups of 16 channels where they divide the stride, else of 8."""
    import inspect
    from latent_feature_grid_compression_amd import ops
    for C, cs, groups in ((5, 8, 1), (13, 16, 1), (22, 24, 3), (30, 32, 2), (8, 8, 1), (32, 32, 2)):
        for L in (2, 4):
            for d in ((5, 9, 12), (2, 56, 56), (1, 1, 1)):
                t = W.cl_target(L, d)
                n = ops._cl_adjoint_groups(L, C, d, t)
                assert n == groups == (cs // 16 if cs % 16 == 0 else cs // 8)
                for drop in (False, True):
                    for cus in CUS:
                        assert plan(lib, True, L, drop, C, d, t, cus)['ngroups'] == n
    src = inspect.getsource(ops._adjoint)
    assert '_cl_adjoint_groups(' in src and '// 16' not in src and '// 8' not in src


# ---- the checker on a chunk that starts without its warm-up planes -------------------------------------------------------

SEAM_D, SEAM_CROP, SEAM_ZCHUNK = (6, 4, 5), (1, 0, 1), 3


def _seam_case(K):
    from latent_feature_grid_compression_amd import ops
    L = 2 * K
    _, frev = W.filters(L)
    bank = ops._factor_bank(frev.numpy())
    t = tuple(2 * v + L - 2 - c for v, c in zip(SEAM_D, SEAM_CROP))
    rng = np.random.default_rng(700 + K)
    return frev, bank, t, rng.standard_normal((2,) + SEAM_D).astype(np.float32), rng.standard_normal((2, 7) + SEAM_D).astype(np.float32)


def test_haar_has_no_seam():
    """K = 1: no carried planes, a chunk has no warm-up to lose."""
    frev, bank, t, lll, hf = _seam_case(1)
    assert np.array_equal(W.separable_level_fp32(lll, hf, bank, t, bug='seam', zchunk=SEAM_ZCHUNK), W.separable_level_fp32(lll, hf, bank, t))


@pytest.mark.parametrize('K', [2, 3])
def test_checker_fails_a_chunk_without_its_warm_up_planes(K):
    """The cell slices jz_begin .. jz_begin + K - 2 of every chunk after the first lose what the coefficient planes
    jz_begin - 1 .. jz_begin - (K - 1) carry into them.  The componentwise checker passes the correct restatement and
    fails the fault at every scale s of the planes those slices are made of (jz_begin - (K - 1) .. jz_begin + K - 2, all
    bands: error and magnitude of the touched voxels shrink together); the max-normalised metric loses it at s = 1e-7."""
    frev, bank, t, lll, hf = _seam_case(K)
    c = W.c_separable(K)
    nz = SEAM_D[0] + K - 1
    begins = list(range(SEAM_ZCHUNK, nz, SEAM_ZCHUNK))
    assert len(begins) == 2
    planes = sorted({p for b in begins for p in range(b - (K - 1), b + K - 1) if 0 <= p < SEAM_D[0]})
    for s, hidden in ((1.0, False), (1e-7, True)):
        l2, h2 = lll.copy(), hf.copy()
        l2[:, planes] *= np.float32(s)
        h2[:, :, planes] *= np.float32(s)
        ref, mag = W.level_reference(torch.from_numpy(l2), torch.from_numpy(h2), frev, t)['out']
        good = W.separable_level_fp32(l2, h2, bank, t)
        bad = W.separable_level_fp32(l2, h2, bank, t, bug='seam', zchunk=SEAM_ZCHUNK)
        touched = np.nonzero((good != bad).any(axis=(0, 2, 3)))[0]
        o0 = (2 * SEAM_D[0] + 2 * K - 2 - t[0]) // 2
        want = sorted({2 * jz + p - o0 for b in begins for jz in range(b, min(b + K - 1, nz)) for p in (0, 1)} & set(range(t[0])))
        assert list(touched) == want                                # exactly the seam slices
        print('K=%d s=%g: seam fault %.3g units, max-normalised %.3g (clean: %.2f units, %.3g)'
              % (K, s, W.worst_ratio(bad, ref, mag), W.rel_err(bad, ref), W.worst_ratio(good, ref, mag), W.rel_err(good, ref)))
        assert W.worst_ratio(good, ref, mag) <= c and W.rel_err(good, ref) <= 1e-6
        assert W.worst_ratio(bad, ref, mag) > 1000 * c
        assert (W.rel_err(bad, ref) <= 1e-6) == hidden
