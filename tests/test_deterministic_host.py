"""CPU tests of the deterministic mode's host side: the quantum rule of the fixed-point grid-gradient scatter against a
restatement in Python integers, and the argument checks of every new C-ABI entry (nothing is launched on these paths:
every row returns before the first kernel)."""
import ctypes
import math

import numpy as np
import pytest

E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4, -5


@pytest.fixture(scope='module')
def lib():
    from latent_feature_grid_compression_amd.build import build
    build(verbose=False)
    from latent_feature_grid_compression_amd import _lib
    return _lib.load()


def _bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def _quantum_exp(max_bits: int, n: int):
    """(E, B) of include/lfgc.h: 2^E >= max with E minimal, B = 61 - ceil(log2(8 n)), in exact integer arithmetic."""
    m = float(np.uint32(max_bits).view(np.float32))          # exact in a double
    f, e = math.frexp(m)                                     # m = f 2^e, 0.5 <= f < 1
    E = e - 1 if f == 0.5 else e
    B = 61 - (8 * n - 1).bit_length()                        # ceil(log2(k)) = (k - 1).bit_length() for k >= 1
    return E, B


def test_quantum_exponent_matches_restatement_and_leaves_headroom(lib):
    maxima = [1, 2, 3, 0x7fffff, 0x800000, 0x800001,         # subnormals (smallest, powers of two and not), first normals
              _bits(1e-30), _bits(1e-12), _bits(0.75), _bits(1.0), _bits(1.0) + 1, _bits(3.0), _bits(4.0), _bits(1e3),
              _bits(65504.0), _bits(3e38), 0x7f7fffff]       # ... up to the largest finite float
    for n in (1, 77, 32768, 2 ** 24, 2 ** 31):
        for mb in maxima:
            E, B = _quantum_exp(mb, n)
            got = lib.lfgc_det_quantum_exp(mb, n)
            assert got == E - B, (hex(mb), n, got, E, B)
            m = float(np.uint32(mb).view(np.float32))
            assert math.ldexp(1.0, E) >= m and math.ldexp(1.0, E - 1) < m          # 2^E >= max, E minimal
            # 8 n contributions of at most 2^E each, in units of q = 2^(E - B): 8 n 2^E / q = 8 n 2^B
            assert 8 * n * 2 ** B < 2 ** 62, (n, B)
            assert 8 * n * 2 ** (B + 1) >= 2 ** 61                                   # and no bit given away beyond that
            assert -207 <= got <= 102                        # 1 / q and q are normal doubles
    # no quantum: all-zero gradients, a non-finite maximum, an empty batch
    for mb, n in ((0, 100), (0x7f800000, 100), (0x7fc00000, 100), (0xffffffff, 100), (_bits(1.0), 0), (_bits(1.0), -3)):
        assert lib.lfgc_det_quantum_exp(mb, n) == 0


def test_backward_det_entries_check_their_arguments(lib):
    from latent_feature_grid_compression_amd import _lib
    ok = _lib.MlpDesc(32, 128, 4, 2, 3, 1)
    bad = _lib.MlpDesc(64, 128, 4, 2, 3, 1)
    plain = lib.lfgc_backward_workspace_bytes(ctypes.byref(ok), 32768)
    det = lib.lfgc_backward_det_workspace_bytes(ctypes.byref(ok), 32768, 64, 64, 64)
    # today's carve (16-byte aligned) + the int64 accumulator (D, H, W, Cs) + the maximum word
    assert det == (plain + 15) // 16 * 16 + 64 ** 3 * 32 * 8 + 16
    small = _lib.MlpDesc(5, 4, 2, 2, 3, 1)
    assert lib.lfgc_backward_det_workspace_bytes(ctypes.byref(small), 77, 3, 4, 5) == \
        (lib.lfgc_backward_workspace_bytes(ctypes.byref(small), 77) + 15) // 16 * 16 + 3 * 4 * 5 * 8 * 8 + 16
    assert lib.lfgc_backward_det_workspace_bytes(ctypes.byref(bad), 100, 8, 8, 8) == E_UNSUPPORTED
    assert lib.lfgc_backward_det_workspace_bytes(None, 100, 8, 8, 8) == E_UNSUPPORTED == lib.lfgc_backward_workspace_bytes(None, 100)
    assert lib.lfgc_backward_det_workspace_bytes(ctypes.byref(ok), -1, 8, 8, 8) == E_SHAPE
    for dims in ((0, 8, 8), (8, 0, 8), (8, 8, -1)):
        assert lib.lfgc_backward_det_workspace_bytes(ctypes.byref(ok), 100, *dims) == E_SHAPE

    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)
    ps = _lib.Positions()
    ps.pos, ps.n = 16, 100
    five, _k1 = _lib.ptr_array([16] * 5)
    hole, _k2 = _lib.ptr_array([16, 16, 0, 16, 16])

    def call(fn, desc=ok, positions=ps, grid=one, dims=(8, 8, 8), packed=one, precision=0, stash=one, d_out=one, d_grid=one,
             dw=five, db=five, ws=one, ws_bytes=1 << 40):
        return fn(ctypes.byref(desc) if desc is not None else None, ctypes.byref(positions) if positions is not None else None,
                  grid, *dims, packed, precision, stash, d_out, d_grid, dw, db, None, ws, ws_bytes, None)

    need = lib.lfgc_backward_det_workspace_bytes(ctypes.byref(ok), 100, 8, 8, 8)
    no_pos = _lib.Positions()
    no_pos.pos, no_pos.n = None, 100
    neg = _lib.Positions()
    neg.pos, neg.n = 16, -1
    for fn in (lib.lfgc_backward_det_f32, lib.lfgc_backward_f32):          # same checks, same order, same codes
        for kw in ('desc', 'positions', 'grid', 'packed', 'stash', 'd_out', 'd_grid', 'dw', 'db'):
            assert call(fn, **{kw: None}) == E_NULL, kw
        assert call(fn, positions=no_pos) == E_NULL
        assert call(fn, dw=hole) == E_NULL and call(fn, db=hole) == E_NULL
        assert call(fn, desc=bad) == E_UNSUPPORTED and call(fn, precision=7) == E_UNSUPPORTED
        assert call(fn, positions=neg) == E_SHAPE and call(fn, dims=(8, 0, 8)) == E_SHAPE
        for kw in ('grid', 'packed', 'stash', 'd_grid', 'ws'):
            assert call(fn, **{kw: odd}) == E_ALIGN, kw
        assert call(fn, ws=None) == E_WORKSPACE and call(fn, ws_bytes=0) == E_WORKSPACE
    assert call(lib.lfgc_backward_det_f32, ws_bytes=need - 1) == E_WORKSPACE
    # the plain scratch alone is not enough for the deterministic entry
    assert call(lib.lfgc_backward_det_f32, ws_bytes=lib.lfgc_backward_workspace_bytes(ctypes.byref(ok), 100)) == E_WORKSPACE


def test_sum_slices_checks_its_arguments(lib):
    one = ctypes.c_void_p(16)
    assert lib.lfgc_sum_slices_f32(None, 2, 8, 8, one, None) == E_NULL
    assert lib.lfgc_sum_slices_f32(one, 2, 8, 8, None, None) == E_NULL
    assert lib.lfgc_sum_slices_f32(one, 0, 8, 8, one, None) == E_SHAPE
    assert lib.lfgc_sum_slices_f32(one, 2, 8, 0, one, None) == E_SHAPE
    assert lib.lfgc_sum_slices_f32(one, 2, 7, 8, one, None) == E_SHAPE          # slices would overlap


def test_stride_zero_drop_adjoints_answer_like_the_plain_entries(lib):
    """Every argument-error row through the plain drop adjoints and through their `_det` forms with slice_stride 0: the same
    code (the plain entries forward with stride 0).  Then the rows only the stride adds."""
    one = ctypes.c_void_p(16)
    taps = (ctypes.c_float * 16)(*[0.5] * 16)
    pg_l1, _k = _lib_ptrs([0, 0, 16, 16])
    pg_l2, _k2 = _lib_ptrs([16, 16, 0, 0])
    ok_cf, ok_cl = (4, 3, 3, 3, 6, 6, 6), (4, 8, 3, 3, 3, 6, 6, 6)

    def cf(det, d_out=one, frev=one, tp=taps, L=4, lll=one, hf=one, ml=one, mh=one, d_lll=one, d_hf=one, dml=one, dmh=one,
           pg=None, shape=ok_cf, stride=0):
        head = (d_out, frev, tp, L, lll, hf, ml, mh, d_lll, d_hf, dml, dmh)
        if det:
            return lib.lfgc_idwt_level_drop_bwd_det_len_f32(*head, stride, pg, *shape, None)
        return lib.lfgc_idwt_level_drop_bwd_len_f32(*head, pg, *shape, None)

    def cl(det, d_out=one, tp=taps, L=4, lll=one, hf=one, ml=one, mh=one, d_lll=one, d_hf=one, dml=one, dmh=one,
           pg=None, shape=ok_cl, stride=0):
        head = (d_out, tp, L, lll, hf, ml, mh, d_lll, d_hf, dml, dmh)
        if det:
            return lib.lfgc_idwt_level_cl_drop_bwd_det_len_f32(*head, stride, pg, *shape, None)
        return lib.lfgc_idwt_level_cl_drop_bwd_len_f32(*head, pg, *shape, None)

    rows_both = [(E_NULL, dict(d_out=None)), (E_NULL, dict(d_lll=None)), (E_NULL, dict(d_hf=None)),
                 (E_NULL, dict(ml=None)), (E_NULL, dict(mh=None)),                     # a factor gradient without its factor
                 (E_NULL, dict(lll=None)), (E_NULL, dict(hf=None)),                    # ... without the coefficients
                 (E_NULL, dict(pg=pg_l1, dml=None, ml=None)), (E_NULL, dict(pg=pg_l1, dmh=None, mh=None)),
                 (E_NULL, dict(pg=pg_l2, lll=None, dml=None, ml=None)),
                 (E_UNSUPPORTED, dict(L=0)), (E_UNSUPPORTED, dict(L=3)), (E_UNSUPPORTED, dict(L=10))]
    for want, kw in rows_both:
        assert cf(False, **kw) == cf(True, **kw) == want, ('channel-first', kw)
        assert cl(False, **kw) == cl(True, **kw) == want, ('channel-last', kw)
    # shapes
    for shape in ((0, 3, 3, 3, 6, 6, 6), (4, 3, 0, 3, 6, 6, 6), (4, 3, 3, 3, 9, 6, 6), (4, 3, 3, 3, 6, 6, 0)):
        assert cf(False, shape=shape) == cf(True, shape=shape) == E_SHAPE, shape
    for shape in ((4, 16, 3, 3, 3, 6, 6, 6), (9, 8, 3, 3, 3, 6, 6, 6), (4, 8, 3, 3, 3, 9, 6, 6), (4, 8, 3, 3, 3, 6, 6, 0)):
        assert cl(False, shape=shape) == cl(True, shape=shape) == E_SHAPE, shape
    # the channel-last pair: 2 and 4 taps, a separable bank, at most 32 channels, arrays below 2^30 bytes
    for kw in (dict(L=6), dict(L=8), dict(tp=None), dict(shape=(40, 40, 3, 3, 3, 6, 6, 6)),
               dict(shape=(32, 32, 200, 200, 200, 400, 400, 400))):
        assert cl(False, **kw) == cl(True, **kw) == E_UNSUPPORTED, kw
    assert cf(False, tp=None, L=6) == cf(True, tp=None, L=6) == E_UNSUPPORTED          # dense stencil: 4 taps only
    # the stride's own rows: negative, or shorter than the larger factor wanted (7 d0 d1 d2 with d_mul_hf, else d0 d1 d2)
    dvol = 27
    for f in (cf, cl):
        assert f(True, stride=-1) == E_SHAPE
        assert f(True, stride=7 * dvol - 1) == E_SHAPE
        assert f(True, stride=dvol - 1, dmh=None) == E_SHAPE
        assert f(True, stride=7 * dvol, d_out=None) == E_NULL                          # the other checks are still the plain entry's
        assert f(True, stride=7 * dvol, L=3) == E_UNSUPPORTED
    assert cl(True, stride=1 << 28) == E_SHAPE


def _lib_ptrs(values):
    from latent_feature_grid_compression_amd import _lib
    return _lib.ptr_array(values)
