"""CPU test of the wavelet launch-plan queries (lfgc_idwt_level_plan, lfgc_idwt_level_bwd_plan, lfgc_dwt_level_plan): the
shapes tests/test_wavelet_paths_gpu.py runs reach the kernel paths it names, the 40 000-voxel switch sits where the
launcher's comment says, and the width limits include/lfgc.h states are the ones the selection functions enforce.  The
launchers consume the structs these queries fill (csrc/lfgc_wavelet.hip), so what is pinned here is what is launched."""
import ctypes

import pytest

from wavelet_bound import ADJOINT_MAX_D2, DB2_PATHS, DENSE_SHAPES, DWT_MAX_N2, ENCODE_SHAPES, SYNTHESIS_MAX_D2, other_length_shapes

OK, E_NULL, E_SHAPE, E_UNSUPPORTED = 0, -1, -2, -3
LDS_CAP = 160 * 1024
LENGTHS = (2, 4, 6, 8)


@pytest.fixture(scope='module')
def lib():
    from latent_feature_grid_compression_amd import _lib
    return _lib.load()


def query(lib, entry, *args):
    """(return code, struct) of a plan entry."""
    from latent_feature_grid_compression_amd import _lib
    info = _lib.WaveletPlanInfo()
    return getattr(lib, entry)(*args, ctypes.byref(info)), info


def full(d, L):
    return tuple(2 * v + L - 2 for v in d)


@pytest.mark.parametrize('name,d,t,kernel,ki,zchunk,gy,length', DB2_PATHS, ids=[c[0] for c in DB2_PATHS])
@pytest.mark.parametrize('drop', [False, True])
def test_db2_shapes_reach_the_named_paths(name, d, t, kernel, ki, zchunk, gy, length, drop):
    from latent_feature_grid_compression_amd import ops
    C = 2
    p = ops.idwt_level_plan(4, C, d, t, has_drop=drop)
    assert (p.kernel, p.ki, p.zchunk, p.len, p.drop) == (kernel, ki, zchunk, length, drop)
    n1, n2 = d[1] + 1, d[2] + 1
    assert p.grid == ((n1 * n2 + 255) // 256, gy, C)
    if kernel == 'sliding_window':
        assert p.ki == (p.len + 255) // 256 and p.lds_bytes == 2 * p.len * 48
        assert gy == -(-(d[0] + 1) // zchunk)
    else:
        assert p.lds_bytes == 2048 + 3 * p.len * 48
    assert p.lds_bytes <= LDS_CAP
    b = ops.idwt_level_bwd_plan(4, C, d, t, has_drop=drop)
    assert (b.kernel, b.drop, b.ki, b.zchunk) == ('analysis_separable', drop, 0, 0)
    assert b.grid == ((d[1] * d[2] + 127) // 128, (d[0] + 1) // 2, C) and b.lds_bytes <= LDS_CAP


def test_the_listed_paths_cover_every_instantiation_and_chunk_remainder():
    """Every (kernel, ki) of the 4-tap separable synthesis, and every way the sliding window's loop (two steps per trip over
    chunks of min(n0, 5) slices) can end: single chunks of 2 and 5, last chunks of 1, 2 and 4."""
    assert {(c[3], c[4]) for c in DB2_PATHS} == {('sliding_window', 1), ('sliding_window', 2), ('sliding_window', 3),
                                                 ('tiled_separable', 0)}
    ends = set()
    for _name, d, _t, kernel, _ki, zchunk, gy, _len in DB2_PATHS:
        if kernel == 'sliding_window':
            n0 = d[0] + 1
            ends.add((gy == 1, n0 - (gy - 1) * zchunk))            # (single chunk, slices of the last chunk)
    assert {(True, 2), (True, 5), (False, 1), (False, 2), (False, 4)} <= ends
    assert max(c[7] for c in DB2_PATHS if c[4] == 1) == 254 and min(c[7] for c in DB2_PATHS if c[4] == 2) == 262
    assert max(c[7] for c in DB2_PATHS if c[4] == 2) == 510 and min(c[7] for c in DB2_PATHS if c[4] == 3) == 514
    assert max(c[7] for c in DB2_PATHS if c[4] == 3) == 762 and min(c[7] for c in DB2_PATHS if c[3] == 'tiled_separable') >= 275


def test_long_rows_take_more_than_64_kb_of_lds():
    from latent_feature_grid_compression_amd import ops
    p = ops.idwt_level_plan(4, 2, (3, 20, 192), (8, 42, 386))
    assert p.kernel == 'tiled_separable' and (p.len + 255) // 256 == 4 and 64 * 1024 < p.lds_bytes <= LDS_CAP


def test_small_level_switch():
    from latent_feature_grid_compression_amd import ops
    assert ops.idwt_level_plan(4, 3, (20, 20, 13), (40, 40, 25)).kernel == 'tiled_separable'      # 40 000 voxels
    assert ops.idwt_level_plan(4, 3, (20, 20, 13), (40, 40, 26)).kernel == 'sliding_window'       # 41 600
    # a dense filter never slides
    assert ops.idwt_level_plan(4, 3, (20, 20, 13), (40, 40, 26), has_taps=False).kernel == 'tiled_dense'


@pytest.mark.parametrize('d,t', DENSE_SHAPES)
def test_dense_shapes(d, t):
    from latent_feature_grid_compression_amd import ops
    assert t[0] * t[1] * t[2] > 40000
    p = ops.idwt_level_plan(4, 2, d, t, has_taps=False)
    assert (p.kernel, p.ki, p.zchunk) == ('tiled_dense', 0, 0) and p.grid[1] == (d[0] + 2) // 2
    assert ops.idwt_level_bwd_plan(4, 2, d, t, has_taps=False).kernel == 'analysis_dense'


@pytest.mark.parametrize('L', [2, 6, 8])
def test_other_lengths_are_tiled_separable(L):
    from latent_feature_grid_compression_amd import ops
    K = L // 2
    for d, t in other_length_shapes(L):
        for drop in (False, True):
            p = ops.idwt_level_plan(L, 2, d, t, has_drop=drop)
            assert (p.kernel, p.ki, p.zchunk, p.drop) == ('tiled_separable', 0, 0, drop)
            assert p.lds_bytes == (K + 1) * p.len * 48 <= LDS_CAP
            assert p.grid == (((d[1] + K - 1) * (d[2] + K - 1) + 255) // 256, (d[0] + K) // 2, 2)
            assert ops.idwt_level_bwd_plan(L, 2, d, t, has_drop=drop).kernel == 'analysis_separable'


@pytest.mark.parametrize('L', LENGTHS)
def test_synthesis_width_limit(lib, L):
    """The last coefficient extent the synthesis takes: every d2 up to the limit of include/lfgc.h (len is not monotone in
    d2, hence the sweep), not the next one; the adjoint and the encode take every level inside it."""
    lim = SYNTHESIS_MAX_D2[L]
    for drop in (0, 1):
        for d2 in range(1, lim + 1):
            d, t = (1, 1, d2), full((1, 1, d2), L)
            rc, p = query(lib, 'lfgc_idwt_level_plan', L, 1, drop, 2, *d, *t)
            assert rc == OK and 0 < p.lds_bytes <= LDS_CAP, (d2, rc, p.lds_bytes)
            assert query(lib, 'lfgc_idwt_level_bwd_plan', L, 1, drop, 2, *d, *t)[0] == OK, d2
        d, t = (1, 1, lim + 1), full((1, 1, lim + 1), L)
        assert query(lib, 'lfgc_idwt_level_plan', L, 1, drop, 2, *d, *t)[0] == E_UNSUPPORTED
        assert query(lib, 'lfgc_idwt_level_plan', L, 1, drop, 2, *d, 1, 1, 1)[0] == E_UNSUPPORTED       # whatever the crop
        assert query(lib, 'lfgc_idwt_level_plan', L, 1, drop, 2, 7, 9, lim + 1, 3, 5, 8)[0] == E_UNSUPPORTED
    for d2 in range(1, lim + 1):
        assert query(lib, 'lfgc_dwt_level_plan', L, 1, 2, L, L, 2 * d2 + L - 2)[0] == OK, d2
    if L == 4:                                                     # the dense stencil stages the same rows
        assert query(lib, 'lfgc_idwt_level_plan', 4, 0, 0, 2, 1, 1, lim, *full((1, 1, lim), 4))[0] == OK
        assert query(lib, 'lfgc_idwt_level_plan', 4, 0, 0, 2, 1, 1, lim + 1, *full((1, 1, lim + 1), 4))[0] == E_UNSUPPORTED


@pytest.mark.parametrize('L', LENGTHS)
def test_encode_width_limit(lib, L):
    """The last source extent the forward DWT takes (the reference's pad-slot quirk makes d2 depend on the parity of n0)."""
    lim = DWT_MAX_N2[L]
    assert lim >= 2 * SYNTHESIS_MAX_D2[L] + L - 2
    for n0 in (2, 3):
        for n2 in range(1, lim + 1):
            rc, p = query(lib, 'lfgc_dwt_level_plan', L, 1, 2, n0, 3, n2)
            assert rc == OK and p.kernel == 4 and 0 < p.lds_bytes <= LDS_CAP, (n0, n2, rc)
    assert E_UNSUPPORTED in {query(lib, 'lfgc_dwt_level_plan', L, 1, 2, n0, 3, lim + 1)[0] for n0 in (2, 3)}


def test_encode_shapes(lib):
    """The encode shapes of the GPU test: the long row is inside the limit for 2 and 4 taps and refused for 6 and 8."""
    from latent_feature_grid_compression_amd import ops
    for L in LENGTHS:
        for n in ENCODE_SHAPES + [(3, 5, 2 * SYNTHESIS_MAX_D2[L] + L - 2)]:
            rc, _ = query(lib, 'lfgc_dwt_level_plan', L, 1, 3, *n)
            assert rc == (OK if n[2] <= DWT_MAX_N2[L] else E_UNSUPPORTED), (L, n)
            if rc == OK:
                p = ops.dwt_level_plan(L, 3, n)
                d = ops.dwt_out_shape(n, L)
                assert p.kernel == 'analysis_separable' and p.grid == ((d[1] * d[2] + 127) // 128, (d[0] + 1) // 2, 3)


def test_plan_queries_report_the_launch_codes(lib):
    """Argument errors come back as from the launch: unsupported lengths, a dense filter of another length, extents."""
    assert lib.lfgc_idwt_level_plan(4, 1, 0, 2, 3, 3, 3, 6, 6, 6, None) == E_NULL
    assert lib.lfgc_idwt_level_bwd_plan(4, 1, 0, 2, 3, 3, 3, 6, 6, 6, None) == E_NULL
    assert lib.lfgc_dwt_level_plan(4, 1, 2, 6, 6, 6, None) == E_NULL
    for entry in ('lfgc_idwt_level_plan', 'lfgc_idwt_level_bwd_plan'):
        for L in (0, 1, 3, 5, 10):
            assert query(lib, entry, L, 1, 0, 2, 3, 3, 3, 6, 6, 6)[0] == E_UNSUPPORTED
        for L in (2, 6, 8):
            assert query(lib, entry, L, 0, 0, 2, 3, 3, 3, 6, 6, 6)[0] == E_UNSUPPORTED
        assert query(lib, entry, 4, 1, 0, 0, 3, 3, 3, 6, 6, 6)[0] == E_SHAPE
        assert query(lib, entry, 4, 1, 0, 2, 3, 3, 3, 9, 6, 6)[0] == E_SHAPE             # t > 2 d + L - 2
        assert query(lib, entry, 8, 1, 0, 2, 3, 3, 3, 12, 12, 12)[0] == OK
        assert query(lib, entry, 4, 1, 0, 2, 3, 0, 3, 6, 6, 6)[0] == E_SHAPE
        assert query(lib, entry, 4, 1, 0, 2, 1024, 1024, 256, 2048, 2048, 512)[0] == E_UNSUPPORTED    # 2^28 coefficients
    assert query(lib, 'lfgc_idwt_level_plan', 4, 1, 0, 70000, 3, 3, 3, 6, 6, 6)[0] == E_UNSUPPORTED
    assert query(lib, 'lfgc_dwt_level_plan', 3, 1, 2, 6, 6, 6)[0] == E_UNSUPPORTED
    assert query(lib, 'lfgc_dwt_level_plan', 6, 0, 2, 6, 6, 6)[0] == E_UNSUPPORTED
    assert query(lib, 'lfgc_dwt_level_plan', 4, 0, 2, 6, 6, 6)[0] == OK
    assert query(lib, 'lfgc_dwt_level_plan', 4, 1, 2, 6, 0, 6)[0] == E_SHAPE
    # the launch agrees where it decides on the host: NULL pointers first, then the same codes
    one = ctypes.c_void_p(16)                                      # any non-NULL address: nothing is launched on these paths
    taps = (ctypes.c_float * 16)(*[0.5] * 16)
    lim = SYNTHESIS_MAX_D2[8]
    assert lib.lfgc_idwt_level_len_f32(one, one, one, taps, 8, one, 2, 1, 1, lim + 1, 8, 8, 2 * lim + 8, None) == E_UNSUPPORTED
    assert lib.lfgc_dwt_level_len_f32(one, one, taps, 8, one, 2, 3, 5, DWT_MAX_N2[8] + 1, None) == E_UNSUPPORTED
    assert lib.lfgc_idwt_level_len_f32(one, one, one, taps, 4, one, 2, 3, 3, 3, 9, 6, 6, None) == E_SHAPE


@pytest.mark.parametrize('L', LENGTHS)
def test_adjoint_width_limit(lib, L):
    """The adjoint's own limit at the full t, beyond the synthesis limit (its staged length grows with d2 there)."""
    lim = ADJOINT_MAX_D2[L]
    assert lim > SYNTHESIS_MAX_D2[L]
    for d2 in range(SYNTHESIS_MAX_D2[L], lim + 1):
        assert query(lib, 'lfgc_idwt_level_bwd_plan', L, 1, 0, 2, 1, 1, d2, *full((1, 1, d2), L))[0] == OK, d2
    assert query(lib, 'lfgc_idwt_level_bwd_plan', L, 1, 0, 2, 1, 1, lim + 1, *full((1, 1, lim + 1), L))[0] == E_UNSUPPORTED


def test_wrappers_name_the_limit():
    """ops._check_level turns the bare LFGC_E_UNSUPPORTED of a channel-first level into a NotImplementedError that names
    the limit the level is over: the width bound of its direction, or the size limits where the width is fine."""
    from latent_feature_grid_compression_amd import ops, _lib
    for L in LENGTHS:
        with pytest.raises(NotImplementedError, match='at most %d for %d taps in the synthesis' % (SYNTHESIS_MAX_D2[L], L)):
            ops._check_level(E_UNSUPPORTED, 'lfgc_idwt_level_drop_len_f32', L, (1, 1, 2000), (2, 2, 4000))
        with pytest.raises(NotImplementedError, match='at most %d for %d taps in the adjoint' % (ADJOINT_MAX_D2[L], L)):
            ops._check_level(E_UNSUPPORTED, 'lfgc_idwt_level_drop_bwd_det_len_f32', L, (1, 1, 2000), (2, 2, 4000), adjoint=True)
        with pytest.raises(NotImplementedError, match='C at most 65535') as e:
            ops._check_level(E_UNSUPPORTED, 'lfgc_idwt_level_drop_len_f32', L, (3, 3, 3), (6, 6, 6))
        assert 'taps' not in str(e.value)
    ops._check_level(OK, 'x', 4, (1, 1, 1), (2, 2, 2))
    with pytest.raises(_lib.LfgcError):
        ops._check_level(E_SHAPE, 'x', 4, (1, 1, 1), (2, 2, 2))
