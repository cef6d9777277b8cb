"""Host-side checks of the channel-last last level with drop layers (lfgc_idwt_level_cl_drop_len_f32 and its adjoint):
the two symbols are exported and bound, and every argument error of include/lfgc.h is reported before anything is launched
(null or dummy pointers, no device work).  No GPU needed."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_UNSUPPORTED = -1, -2, -3
NAN = float('nan')


@pytest.fixture(scope='module')
def lib():
    from latent_feature_grid_compression_amd.build import build
    from latent_feature_grid_compression_amd import _lib
    build(verbose=False)
    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    from latent_feature_grid_compression_amd import _lib, ops
    raw = ctypes.CDLL(os.path.join(ROOT, 'latent_feature_grid_compression_amd', 'liblfgc.so'))
    for name in ('lfgc_idwt_level_cl_drop_len_f32', 'lfgc_idwt_level_cl_drop_bwd_len_f32'):
        assert hasattr(raw, name)
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES['lfgc_idwt_level_cl_drop_len_f32'][1]) == 18
    assert len(_lib.SIGNATURES['lfgc_idwt_level_cl_drop_bwd_len_f32'][1]) == 21
    assert callable(ops.idwt_level_cl_drop) and callable(ops.idwt_level_cl_drop_bwd)


def test_forward_return_codes(lib):
    f = lib.lfgc_idwt_level_cl_drop_len_f32
    one = ctypes.c_void_p(16)                            # any non-NULL address: nothing is launched on these paths
    for L in (2, 4):
        taps = (ctypes.c_float * (2 * L))(*[0.5] * (2 * L))
        full = 2 * 3 + L - 2                             # largest t_a for d_a = 3
        # a required pointer is missing (the factors are optional)
        assert f(None, one, one, NAN, one, NAN, taps, L, one, 4, 8, 3, 3, 3, 6, 6, 6, None) == E_NULL
        assert f(one, None, one, NAN, one, NAN, taps, L, one, 4, 8, 3, 3, 3, 6, 6, 6, None) == E_NULL
        assert f(one, one, one, NAN, one, NAN, taps, L, None, 4, 8, 3, 3, 3, 6, 6, 6, None) == E_NULL
        # channel stride is not C rounded up to 8; t_a out of range
        assert f(one, one, one, NAN, one, NAN, taps, L, one, 4, 16, 3, 3, 3, 6, 6, 6, None) == E_SHAPE
        assert f(one, one, one, NAN, one, NAN, taps, L, one, 9, 8, 3, 3, 3, 6, 6, 6, None) == E_SHAPE
        assert f(one, one, one, NAN, one, NAN, taps, L, one, 4, 8, 3, 3, 3, full + 1, 6, 6, None) == E_SHAPE
        assert f(one, one, one, NAN, one, NAN, taps, L, one, 4, 8, 3, 3, 3, 6, 6, 0, None) == E_SHAPE
        # dense stencil, C > 32, an array of 2^30 bytes and more
        assert f(one, one, one, NAN, one, NAN, None, L, one, 4, 8, 3, 3, 3, 6, 6, 6, None) == E_UNSUPPORTED
        assert f(one, one, one, NAN, one, NAN, taps, L, one, 40, 40, 3, 3, 3, 6, 6, 6, None) == E_UNSUPPORTED
        assert f(one, one, None, NAN, None, NAN, taps, L, one, 33, 40, 3, 3, 3, 6, 6, 6, None) == E_UNSUPPORTED
        assert f(one, one, one, NAN, one, NAN, taps, L, one, 32, 32, 200, 200, 200, 400, 400, 400, None) == E_UNSUPPORTED
        assert f(one, one, one, NAN, one, NAN, taps, L, one, 32, 32, 110, 110, 110, 6, 6, 6, None) == E_UNSUPPORTED
    taps8 = (ctypes.c_float * 16)(*[0.5] * 16)
    for L in (0, 1, 3, 6, 8):
        assert f(one, one, one, NAN, one, NAN, taps8, L, one, 4, 8, 3, 3, 3, 6, 6, 6, None) == E_UNSUPPORTED


def test_adjoint_return_codes(lib):
    from latent_feature_grid_compression_amd import _lib
    b = lib.lfgc_idwt_level_cl_drop_bwd_len_f32
    one = ctypes.c_void_p(16)
    shape = (4, 8, 3, 3, 3, 6, 6, 6, None)

    def pens(*which):                                    # host array of 4 device pointers, the named slots non-NULL
        arr, _keep = _lib.ptr_array([16 if i in which else 0 for i in range(4)])
        return arr

    for L in (2, 4):
        taps = (ctypes.c_float * (2 * L))(*[0.5] * (2 * L))
        # required: the incoming gradient and both coefficient gradients
        assert b(None, taps, L, one, one, one, one, one, one, one, one, None, *shape) == E_NULL
        assert b(one, taps, L, one, one, one, one, None, one, one, one, None, *shape) == E_NULL
        assert b(one, taps, L, one, one, one, one, one, None, one, one, None, *shape) == E_NULL
        # a factor gradient needs its factor and its coefficients
        assert b(one, taps, L, one, one, None, one, one, one, one, None, None, *shape) == E_NULL      # d_mul_lll, no mul_lll
        assert b(one, taps, L, None, one, one, one, one, one, one, None, None, *shape) == E_NULL      # d_mul_lll, no lll
        assert b(one, taps, L, one, one, one, None, one, one, None, one, None, *shape) == E_NULL      # d_mul_hf, no mul_hf
        assert b(one, taps, L, one, None, one, one, one, one, None, one, None, *shape) == E_NULL      # d_mul_hf, no hf
        # an L2 penalty needs the coefficients, an L1 penalty the factor gradient it is added to
        assert b(one, taps, L, None, one, None, None, one, one, None, None, pens(0), *shape) == E_NULL
        assert b(one, taps, L, one, None, None, None, one, one, None, None, pens(1), *shape) == E_NULL
        assert b(one, taps, L, one, one, one, one, one, one, None, one, pens(2), *shape) == E_NULL
        assert b(one, taps, L, one, one, one, one, one, one, one, None, pens(3), *shape) == E_NULL
        # shapes
        assert b(one, taps, L, one, one, one, one, one, one, one, one, None, 4, 16, 3, 3, 3, 6, 6, 6, None) == E_SHAPE
        assert b(one, taps, L, one, one, one, one, one, one, one, one, None, 4, 8, 3, 3, 3, 6, 2 * 3 + L - 1, 6, None) == E_SHAPE
        # dense stencil, C > 32, arrays of 2^30 bytes and more
        assert b(one, None, L, one, one, one, one, one, one, one, one, None, *shape) == E_UNSUPPORTED
        assert b(one, taps, L, one, one, one, one, one, one, one, one, None, 40, 40, 3, 3, 3, 6, 6, 6, None) == E_UNSUPPORTED
        assert b(one, taps, L, one, one, one, one, one, one, one, one, None, 32, 32, 200, 200, 200, 400, 400, 400, None) == E_UNSUPPORTED
    taps8 = (ctypes.c_float * 16)(*[0.5] * 16)
    for L in (0, 3, 6, 8):
        assert b(one, taps8, L, one, one, one, one, one, one, one, one, None, *shape) == E_UNSUPPORTED
