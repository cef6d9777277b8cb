"""Tensor-level wrappers over the C-ABI (device memory and streams come from PyTorch-ROCm; all
arithmetic happens in liblfgc.so) and the two autograd Functions of the hot path."""
from __future__ import annotations

import contextlib
import ctypes
import functools
import os
import struct
import threading
import weakref
from types import SimpleNamespace
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import MlpDesc, Positions, check


_DEBUG_STATUS = bool(os.environ.get('LFGC_DEBUG_STATUS'))


def _require_hip(*tensors: torch.Tensor) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.LfgcError('the latent-feature-grid hot path runs on the MI355X only: got a %s tensor. '
                                 'Move the module and its inputs to the GPU (model.cuda()); there is no CPU fallback.'
                                 % t.device)


def _stream(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _cuda_tensors(objs):
    for o in objs:
        if torch.is_tensor(o):
            if o.is_cuda:
                yield o
        elif isinstance(o, (list, tuple)):
            yield from _cuda_tensors(o)


def _on_device(fn):
    """Run a wrapper with the device of its tensor arguments current.  The library launches on the calling thread's
    CURRENT device (and keeps its per-device caches by it), while the stream handle passed down belongs to the tensors'
    device: a model on cuda:1 called while cuda:0 is current would otherwise launch on the wrong device.  Tensors living
    on different devices are refused."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        dev = None
        for t in _cuda_tensors(list(args) + list(kwargs.values())):
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise _lib.LfgcError('tensors on different devices (%s and %s) in one call of %s' % (dev, t.device, fn.__name__))
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapped


# ---- deterministic mode ----------------------------------------------------------------------------------
# Bitwise repeatable gradients: the grid gradient is scattered in 64-bit fixed point and the drop
# factors' gradients get one writer per address.  The autograd nodes below read the mode once, in their forward, and keep it
# in their ctx for the backward; their apply() signatures do not carry it.

_MODE = threading.local()


def deterministic_enabled() -> bool:
    """The mode the autograd nodes built right now will run their backward in: the innermost deterministic_mode() of this
    thread, else torch.are_deterministic_algorithms_enabled()."""
    forced = getattr(_MODE, 'forced', None)
    return torch.are_deterministic_algorithms_enabled() if forced is None else forced


@contextlib.contextmanager
def deterministic_mode(flag: Optional[bool]):
    """Force the mode on (True) or off (False) for the nodes built inside; None follows the torch global."""
    before = getattr(_MODE, 'forced', None)
    _MODE.forced = None if flag is None else bool(flag)
    try:
        yield
    finally:
        _MODE.forced = before


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def make_desc(C: int, H: int, L: int, n_freqs: int, d_in: int = 3, d_out: int = 1) -> MlpDesc:
    d = MlpDesc(int(C), int(H), int(L), int(n_freqs), int(d_in), int(d_out))
    if not _lib.load().lfgc_mlp_supported(ctypes.byref(d)):
        raise _lib.LfgcError('network shape not covered by the compiled HIP kernels: grid_channels=%d (<=32), hidden=%d '
                             '(<=128), num_layer=%d (<=8), n_freqs=%d (==2), d_in=%d (==3), d_out=%d (==1)'
                             % (C, H, L, n_freqs, d_in, d_out))
    return d


def grid_channel_stride(C: int) -> int:
    return int(_lib.load().lfgc_grid_channel_stride(int(C)))


# ---- wavelet levels ------------------------------------------------------------------------------------

_TAPS_CACHE = {}      # id(filter tensor) -> (weakref, version, ctypes float[2L] or None)
FILTER_LENGTHS = (2, 4, 6, 8)      # even filter lengths the HIP kernels take (include/lfgc.h: lfgc_idwt_level_len_f32)


def filter_length(filt: torch.Tensor) -> int:
    """L of an (8, L,L,L) wavelet filter buffer."""
    L = int(filt.shape[-1])
    if L not in FILTER_LENGTHS:
        raise NotImplementedError('the HIP wavelet kernels take filter lengths %s, got %d' % (FILTER_LENGTHS, L))
    return L


def _outer_bank(a: np.ndarray) -> np.ndarray:
    """(2,L) fp32 taps -> (8,L,L,L) fp32 the way the reference forms it: a[sz][tz] * (a[sy][ty] * a[sx][tx]), s = 4sz+2sy+sx
    (wavelet_transform/Torch_Wavelet_Transform.py:44-53)."""
    a = a.astype(np.float32)
    L = a.shape[-1]
    yx = (a[:, None, :, None] * a[None, :, None, :]).astype(np.float32)               # [sy][sx][ty][tx]
    out = (a[:, None, None, :, None, None] * yx[None, :, :, None, :, :]).astype(np.float32)   # [sz][sy][sx][tz][ty][tx]
    return out.reshape(8, L, L, L)


def _factor_bank(f3d: np.ndarray) -> Optional[np.ndarray]:
    """1-D bank (2,L) whose outer product IS the given (8,L,L,L) filter, or None if the filter is not separable."""
    L = f3d.shape[-1]
    f3d = f3d.astype(np.float32).reshape(8, L, L, L)
    c = float(f3d[0, 0, 0, 0])
    if c == 0.0 or not np.isfinite(f3d).all():
        return None
    a0 = np.cbrt(np.float64(c))
    a = (f3d[[0, 1], 0, 0, :].astype(np.float64) / (a0 * a0)).astype(np.float32)      # bands (0,0,sx), taps along x
    # exact fp32 taps are within an ulp or two of this estimate: search the neighbours for a bit-exact reconstruction
    best, best_err = None, np.inf
    for d_lo in (0, -1, 1, -2, 2):
        for d_hi in (0, -1, 1, -2, 2):
            cand = a.copy()
            for row, d in ((0, d_lo), (1, d_hi)):
                for _ in range(abs(d)):
                    cand[row] = np.nextafter(cand[row], np.float32(np.inf) if d > 0 else np.float32(-np.inf))
            err = float(np.abs(_outer_bank(cand) - f3d).max())
            if err < best_err:
                best, best_err = cand, err
            if err == 0.0:
                return cand
    scale = float(np.abs(f3d).max())
    return best if best_err <= 4e-7 * scale else None


def filter_taps(filt: torch.Tensor):
    """ctypes float[2L] = the 1-D bank of a wavelet filter buffer (or None: not separable -> dense stencil, 4 taps only).
    Costs one device-to-host copy of the buffer the first time it is seen; cached per tensor object and in-place version."""
    ent = _TAPS_CACHE.get(id(filt))
    if ent is not None and ent[0]() is filt and ent[1] == filt._version:
        return ent[2]
    bank = _factor_bank(filt.detach().float().cpu().numpy())
    taps = None if bank is None else (ctypes.c_float * bank.size)(*[float(v) for v in bank.reshape(-1)])
    if len(_TAPS_CACHE) > 256:
        for k in [k for k, e in _TAPS_CACHE.items() if e[0]() is None]:
            del _TAPS_CACHE[k]
    _TAPS_CACHE[id(filt)] = (weakref.ref(filt), filt._version, taps)
    return taps


_E_UNSUPPORTED = -3
_NAN = float('nan')
# Width limits of the channel-first level kernels per filter length (include/lfgc.h: lfgc_idwt_level_len_f32; a workgroup
# stages whole rows in 160 KB of LDS): the largest last coefficient extent d2 the synthesis takes, the same for the adjoint
# at the full t, and the largest last source extent n2 of the forward DWT
SYNTHESIS_MAX_D2 = {2: 853, 4: 373, 6: 169, 8: 96}
ADJOINT_MAX_D2 = {2: 1280, 4: 560, 6: 318, 8: 201}
DWT_MAX_N2 = {2: 2560, 4: 1122, 6: 638, 8: 408}


def _check_level(code: int, what: str, L: int, d: Sequence[int], t: Sequence[int], adjoint: bool = False) -> None:
    """check() for the channel-first level entries: LFGC_E_UNSUPPORTED becomes a NotImplementedError that names the limit
    the level is over -- the width bound of its direction where d2 exceeds it, else the size limits of a launch."""
    if code == _E_UNSUPPORTED:
        table = ADJOINT_MAX_D2 if adjoint else SYNTHESIS_MAX_D2
        if d[2] > SYNTHESIS_MAX_D2[L]:
            why = ('the last coefficient extent d2 may be at most %d for %d taps in the %s (whole rows are staged in LDS)'
                   % (table[L], L, 'adjoint at the full t; the synthesis takes at most %d' % SYNTHESIS_MAX_D2[L]
                      if adjoint else 'synthesis'))
        else:
            why = 'a channel holds fewer than 2^28 coefficients and 2^31 outputs, d0 is below 2^17 and C at most 65535'
        raise NotImplementedError('%s: level d=%s -> t=%s is outside the channel-first wavelet kernels: %s'
                                  % (what, tuple(d), tuple(t), why))
    check(code, what)


def _thr(v) -> float:
    return _NAN if v is None else float(v)


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def _cl_level_ok(C: int, d: Sequence[int], t: Sequence[int], taps, L: int = 4) -> bool:
    """Shapes the channel-last last-level kernels take (lfgc.h: lfgc_idwt_level_cl_f32): separable bank of 2 or 4 taps,
    C <= 32, arrays below 2^30 bytes.  Anything else composes the channel-first level with the layout conversion."""
    if taps is None or L not in (2, 4) or C > 32 or os.environ.get('LFGC_CL_LEVEL', '1') == '0':
        return False
    cs = grid_channel_stride(C)
    return t[0] * t[1] * t[2] * cs * 4 < (1 << 30) and d[0] * d[1] * d[2] * 7 * C * 4 < (1 << 30)


def _level_shapes(C: int, d: Sequence[int]) -> dict:
    d = tuple(int(v) for v in d)
    return {'lll': (C,) + d, 'hf': (C, 7) + d, 'mul_l': d, 'mul_h': (7,) + d}


def _synthesis(lll, hf, filter_rev, target, mul_l=None, thr_l=None, mul_h=None, thr_h=None, channel_last=False):
    """One IDWT level, every variant: lll (C,d0,d1,d2), hf (C,7,d0,d1,d2), optional drop factors mul_l (d0,d1,d2) /
    mul_h (7,d0,d1,d2) with their thresholds (include/lfgc.h) -> (C,t0,t1,t2), or with channel_last the sampler's
    (t0,t1,t2,Cs) grid.  The kernels take raw addresses: every tensor becomes contiguous fp32 of exactly the level's
    shape here.  Shapes the channel-last kernels do not take (_cl_level_ok) run channel-first behind to_channel_last."""
    _require_hip(lll, hf, filter_rev, mul_l, mul_h)
    taps = filter_taps(filter_rev)
    L = filter_length(filter_rev)
    C, d0, d1, d2 = lll.shape
    shapes = _level_shapes(C, (d0, d1, d2))
    if tuple(hf.shape) != shapes['hf']:
        raise ValueError('detail bands %s do not match low band %s' % (tuple(hf.shape), tuple(lll.shape)))
    if mul_l is not None and tuple(mul_l.shape) != shapes['mul_l']:
        raise ValueError('low-band drop factor %s does not match %s' % (tuple(mul_l.shape), shapes['mul_l']))
    if mul_h is not None and tuple(mul_h.shape) != shapes['mul_h']:
        raise ValueError('detail drop factor %s does not match %s' % (tuple(mul_h.shape), shapes['mul_h']))
    lll, hf = _f32c(lll), _f32c(hf)
    mul_l = _f32c(mul_l) if mul_l is not None else None
    mul_h = _f32c(mul_h) if mul_h is not None else None
    t = [int(v) for v in target]
    if channel_last and _cl_level_ok(C, (d0, d1, d2), t, taps, L):
        cs = grid_channel_stride(C)
        out = torch.empty((t[0], t[1], t[2], cs), dtype=torch.float32, device=lll.device)
        check(_lib.load().lfgc_idwt_level_cl_drop_len_f32(
            lll.data_ptr(), hf.data_ptr(), _ptr(mul_l), _thr(thr_l), _ptr(mul_h), _thr(thr_h), taps, L, out.data_ptr(),
            C, cs, d0, d1, d2, t[0], t[1], t[2], _stream(lll)), 'lfgc_idwt_level_cl_drop_len_f32')
        return out
    filter_rev = _f32c(filter_rev)
    out = torch.empty((C, t[0], t[1], t[2]), dtype=torch.float32, device=lll.device)
    _check_level(_lib.load().lfgc_idwt_level_drop_len_f32(
        lll.data_ptr(), hf.data_ptr(), _ptr(mul_l), _thr(thr_l), _ptr(mul_h), _thr(thr_h), filter_rev.data_ptr(), taps, L,
        out.data_ptr(), C, d0, d1, d2, t[0], t[1], t[2], _stream(lll)), 'lfgc_idwt_level_drop_len_f32', L, (d0, d1, d2), t)
    return to_channel_last(out) if channel_last else out


def _adjoint(d_out, C, filter_rev, lll, hf, mul_l, mul_h, want_dml, want_dmh, d, penalty_ptrs, channel_last,
             deterministic=False):
    """Adjoint of _synthesis -> (d_lll, d_hf, d_mul_l or None, d_mul_h or None).  d_out (C,t0,t1,t2), or with
    channel_last (t0,t1,t2,Cs) and C given.  lll / hf / mul_l / mul_h: the forward's inputs as far as the factor and
    penalty gradients need them, else None.  want_dml / want_dmh: False, True (a zero tensor is allocated) or a
    ZERO-FILLED tensor of the factor's shape to accumulate into.  penalty_ptrs: None or 4 device addresses (0 = none) of
    the upstream gradients of [sum lll^2, sum hf^2, sum |mul_l|, sum |mul_h|] whose own gradients the kernel folds in
    (include/lfgc.h).  deterministic: every address of a factor gradient gets one writer -- the kernels write S slices
    (channel-first: one per channel; channel-last: one per channel group) of a zero-filled S x factor scratch, which
    lfgc_sum_slices_f32 folds in slice order (S == 1 is that already)."""
    _require_hip(d_out, filter_rev, lll, hf, mul_l, mul_h)
    taps = filter_taps(filter_rev)
    L = filter_length(filter_rev)
    d = [int(v) for v in d]
    if channel_last:
        t0, t1, t2, cs = d_out.shape
    else:
        C, t0, t1, t2 = d_out.shape
    # the kernels take raw addresses: contiguous fp32 of exactly the level's shapes
    shapes = _level_shapes(C, d)
    given = {'lll': lll, 'hf': hf, 'mul_l': mul_l, 'mul_h': mul_h}
    for name, x in given.items():
        if x is not None:
            if tuple(x.shape) != shapes[name]:
                raise ValueError('%s %s does not match the level %s' % (name, tuple(x.shape), shapes[name]))
            given[name] = _f32c(x)
    for name, x in (('mul_l', want_dml), ('mul_h', want_dmh)):
        if torch.is_tensor(x) and (tuple(x.shape) != shapes[name] or x.dtype != torch.float32 or not x.is_contiguous()):
            raise ValueError('gradient buffer of %s must be contiguous fp32 of shape %s' % (name, shapes[name]))
    use_cl = channel_last and _cl_level_ok(C, d, (t0, t1, t2), taps, L)
    if use_cl and cs != grid_channel_stride(C):
        raise ValueError('gradient grid %s is not the channel-last grid of %d channels' % (tuple(d_out.shape), C))
    d_out = _f32c(to_channel_first(d_out, C) if (channel_last and not use_cl) else d_out)
    dev = d_out.device
    d_lll = torch.empty(shapes['lll'], dtype=torch.float32, device=dev)
    d_hf = torch.empty(shapes['hf'], dtype=torch.float32, device=dev)
    d_ml = want_dml if torch.is_tensor(want_dml) else (
        torch.zeros(shapes['mul_l'], dtype=torch.float32, device=dev) if want_dml else None)
    d_mh = want_dmh if torch.is_tensor(want_dmh) else (
        torch.zeros(shapes['mul_h'], dtype=torch.float32, device=dev) if want_dmh else None)
    pen, _keep = (None, None) if penalty_ptrs is None else _lib.ptr_array([int(v) for v in penalty_ptrs])
    # slices of the deterministic mode: the channel groups the channel-last adjoint's own selection runs
    nslices, stride, sl, sh = 1, 0, d_ml, d_mh
    if deterministic and (d_ml is not None or d_mh is not None):
        nslices = _cl_adjoint_groups(L, C, d, (t0, t1, t2)) if use_cl else C
    if nslices > 1:
        stride = int(np.prod(shapes['mul_h' if d_mh is not None else 'mul_l']))
        sl = torch.zeros((nslices, stride), dtype=torch.float32, device=dev) if d_ml is not None else None
        sh = torch.zeros((nslices, stride), dtype=torch.float32, device=dev) if d_mh is not None else None
    operands = (_ptr(given['lll']), _ptr(given['hf']), _ptr(given['mul_l']), _ptr(given['mul_h']), d_lll.data_ptr(),
                d_hf.data_ptr(), _ptr(sl), _ptr(sh), stride, pen, C)
    if use_cl:
        check(_lib.load().lfgc_idwt_level_cl_drop_bwd_det_len_f32(
            d_out.data_ptr(), taps, L, *operands, cs, d[0], d[1], d[2], t0, t1, t2, _stream(d_out)),
            'lfgc_idwt_level_cl_drop_bwd_det_len_f32')
    else:
        filter_rev = _f32c(filter_rev)
        _check_level(_lib.load().lfgc_idwt_level_drop_bwd_det_len_f32(
            d_out.data_ptr(), filter_rev.data_ptr(), taps, L, *operands, d[0], d[1], d[2], t0, t1, t2, _stream(d_out)),
            'lfgc_idwt_level_drop_bwd_det_len_f32', L, d, (t0, t1, t2), adjoint=True)
    if stride:
        for slices, out in ((sl, d_ml), (sh, d_mh)):
            if out is not None:
                check(_lib.load().lfgc_sum_slices_f32(slices.data_ptr(), nslices, stride, out.numel(), out.data_ptr(),
                                                      _stream(d_out)), 'lfgc_sum_slices_f32')
    return d_lll, d_hf, d_ml, d_mh


@_on_device
def idwt_level(lll: torch.Tensor, hf: torch.Tensor, filter_rev: torch.Tensor, target: Sequence[int]) -> torch.Tensor:
    """lll (C,d0,d1,d2), hf (C,7,d0,d1,d2) -> (C,t0,t1,t2)."""
    return _synthesis(lll, hf, filter_rev, target)


@_on_device
def idwt_level_bwd(d_out: torch.Tensor, filter_rev: torch.Tensor, d: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """d_out (C,t0,t1,t2) -> (d_lll (C,d0,d1,d2), d_hf (C,7,d0,d1,d2))."""
    return _adjoint(d_out, None, filter_rev, None, None, None, None, False, False, d, None, False)[:2]


@_on_device
def idwt_level_cl(lll: torch.Tensor, hf: torch.Tensor, filter_rev: torch.Tensor, target: Sequence[int]) -> torch.Tensor:
    """lll (C,d0,d1,d2), hf (C,7,d0,d1,d2) -> (t0,t1,t2,Cs) channel-last, pad channels zero: the last level of the
    decode and the layout conversion in one kernel (falls back to the two-kernel form for shapes it does not take)."""
    return _synthesis(lll, hf, filter_rev, target, channel_last=True)


@_on_device
def idwt_level_cl_bwd(d_out_cl: torch.Tensor, C: int, filter_rev: torch.Tensor,
                      d: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """d_out_cl (t0,t1,t2,Cs) -> (d_lll (C,d0,d1,d2), d_hf (C,7,d0,d1,d2)): adjoint of idwt_level_cl."""
    return _adjoint(d_out_cl, C, filter_rev, None, None, None, None, False, False, d, None, True)[:2]


# The pruning ("drop") layers fused into the level

@_on_device
def idwt_level_drop(lll, hf, mul_l, thr_l, mul_h, thr_h, filter_rev, target) -> torch.Tensor:
    """One IDWT level with the drop factors of its inputs folded in: mul_l (d0,d1,d2) / mul_h (7,d0,d1,d2) or None;
    thr None = plain product, a float = masked straight-through rule (see include/lfgc.h)."""
    return _synthesis(lll, hf, filter_rev, target, mul_l, thr_l, mul_h, thr_h)


@_on_device
def idwt_level_drop_bwd(d_out, filter_rev, lll, hf, mul_l, mul_h, want_dml, want_dmh, d, penalty_ptrs=None):
    """Adjoint of idwt_level_drop -> (d_lll, d_hf, d_mul_l or None, d_mul_h or None).  want_dml / want_dmh: False, True
    (a zero tensor is allocated) or a ZERO-FILLED tensor of the factor's shape to accumulate into.  penalty_ptrs: None or
    4 device addresses (0 = none) of the upstream gradients of [sum lll^2, sum hf^2, sum |mul_l|, sum |mul_h|] whose own
    gradients the kernel folds in (include/lfgc.h)."""
    return _adjoint(d_out, None, filter_rev, lll, hf, mul_l, mul_h, want_dml, want_dmh, d, penalty_ptrs, False)


@_on_device
def idwt_level_cl_drop(lll, hf, mul_l, thr_l, mul_h, thr_h, filter_rev, target) -> torch.Tensor:
    """idwt_level_drop writing the sampler's channel-last grid (t0,t1,t2,Cs), pad channels zero: the last level of a
    decode with drop layers and the layout conversion in one kernel (falls back to the two-kernel form for shapes the
    channel-last kernels do not take, see _cl_level_ok)."""
    return _synthesis(lll, hf, filter_rev, target, mul_l, thr_l, mul_h, thr_h, channel_last=True)


@_on_device
def idwt_level_cl_drop_bwd(d_out_cl, C, filter_rev, lll, hf, mul_l, mul_h, want_dml, want_dmh, d, penalty_ptrs=None):
    """Adjoint of idwt_level_cl_drop: d_out_cl (t0,t1,t2,Cs) -> (d_lll, d_hf, d_mul_l or None, d_mul_h or None), the
    arguments of idwt_level_drop_bwd (falls back to it behind the layout conversion like idwt_level_cl_drop)."""
    return _adjoint(d_out_cl, C, filter_rev, lll, hf, mul_l, mul_h, want_dml, want_dmh, d, penalty_ptrs, True)


@_on_device
def to_channel_last(grid_cf: torch.Tensor) -> torch.Tensor:
    """(C,D,H,W) -> (D,H,W,Cs), Cs = C rounded up to 8, pad channels zero."""
    _require_hip(grid_cf)
    grid_cf = _f32c(grid_cf)
    C, D, H, W = grid_cf.shape
    cs = grid_channel_stride(C)
    out = torch.empty((D, H, W, cs), dtype=torch.float32, device=grid_cf.device)
    check(_lib.load().lfgc_grid_layout_f32(grid_cf.data_ptr(), out.data_ptr(), C, D * H * W, cs, 1, _stream(grid_cf)),
          'lfgc_grid_layout_f32')
    return out


@_on_device
def to_channel_first(grid_cl: torch.Tensor, C: int) -> torch.Tensor:
    """(D,H,W,Cs) -> (C,D,H,W)."""
    _require_hip(grid_cl)
    grid_cl = _f32c(grid_cl)
    D, H, W, cs = grid_cl.shape
    out = torch.empty((C, D, H, W), dtype=torch.float32, device=grid_cl.device)
    check(_lib.load().lfgc_grid_layout_f32(grid_cl.data_ptr(), out.data_ptr(), C, D * H * W, cs, 0, _stream(grid_cl)),
          'lfgc_grid_layout_f32')
    return out


def dwt_out_shape(n: Sequence[int], L: int = 4) -> List[int]:
    n = [int(v) for v in n]
    lo = (2 * L - 3) // 2
    hi = [lo + (n[2] & 1), lo + (n[1] & 1), lo + (n[0] & 1)]     # reference pad-slot quirk, see lfgc.h
    return [(n[a] + lo + hi[a] - L) // 2 + 1 for a in range(3)]


@_on_device
def dwt_level(data: torch.Tensor, filter_fwd: torch.Tensor) -> torch.Tensor:
    """data (C,n0,n1,n2) -> (C,8,d0,d1,d2)."""
    _require_hip(data, filter_fwd)
    taps = filter_taps(filter_fwd)
    data, filter_fwd = _f32c(data), _f32c(filter_fwd)
    C, n0, n1, n2 = data.shape
    L = filter_length(filter_fwd)
    d = dwt_out_shape((n0, n1, n2), L)
    out = torch.empty((C, 8, d[0], d[1], d[2]), dtype=torch.float32, device=data.device)
    code = _lib.load().lfgc_dwt_level_len_f32(data.data_ptr(), filter_fwd.data_ptr(), taps, L, out.data_ptr(), C, n0, n1, n2,
                                              _stream(data))
    if code == _E_UNSUPPORTED:
        raise NotImplementedError('lfgc_dwt_level_len_f32: input %s is outside the forward-DWT kernel: %s' % (
            (n0, n1, n2), 'the last extent n2 may be at most %d for %d taps (whole rows are staged in LDS)' % (DWT_MAX_N2[L], L)
            if n2 > DWT_MAX_N2[L] else 'a channel holds fewer than 2^31 values, n0 is below 2^17 and C at most 65535'))
    check(code, 'lfgc_dwt_level_len_f32')
    return out


def _wavelet_plan(entry: str, *args) -> SimpleNamespace:
    info = _lib.WaveletPlanInfo()
    check(getattr(_lib.load(), entry)(*[int(v) for v in args], ctypes.byref(info)), entry)
    return SimpleNamespace(kernel=_lib.WAVELET_KERNELS[info.kernel], drop=bool(info.drop), ki=int(info.ki),
                           zchunk=int(info.zchunk), len=int(info.len), lds_bytes=int(info.lds_bytes),
                           grid=tuple(int(v) for v in info.grid))


def idwt_level_plan(filter_len: int, C: int, d: Sequence[int], t: Sequence[int], has_taps: bool = True,
                    has_drop: bool = False) -> SimpleNamespace:
    """lfgc_idwt_level_plan: the launch idwt_level / idwt_level_drop (has_drop) would make for a level d -> t of C channels,
    nothing enqueued, no device needed.  has_taps: the filter is separable (filter_taps() is not None).  Fields: kernel
    (a name of _lib.WAVELET_KERNELS), drop, ki, zchunk, len, lds_bytes, grid (x, y, z workgroups)."""
    return _wavelet_plan('lfgc_idwt_level_plan', filter_len, has_taps, has_drop, C, *d, *t)


def idwt_level_bwd_plan(filter_len: int, C: int, d: Sequence[int], t: Sequence[int], has_taps: bool = True,
                        has_drop: bool = False) -> SimpleNamespace:
    """lfgc_idwt_level_bwd_plan: the same for idwt_level_bwd / idwt_level_drop_bwd (has_drop: factors or L2 penalties)."""
    return _wavelet_plan('lfgc_idwt_level_bwd_plan', filter_len, has_taps, has_drop, C, *d, *t)


def dwt_level_plan(filter_len: int, C: int, n: Sequence[int], has_taps: bool = True) -> SimpleNamespace:
    """lfgc_dwt_level_plan: the same for dwt_level of a (C, n0,n1,n2) input."""
    return _wavelet_plan('lfgc_dwt_level_plan', filter_len, has_taps, C, *n)


def _wavelet_cl_plan(entry: str, filter_len, has_drop, C, d, t, num_cus) -> SimpleNamespace:
    info = _lib.WaveletClPlanInfo()
    check(getattr(_lib.load(), entry)(int(filter_len), int(bool(has_drop)), int(C), grid_channel_stride(C),
                                      *[int(v) for v in d], *[int(v) for v in t], int(num_cus), ctypes.byref(info)), entry)
    p = SimpleNamespace(**{k: int(getattr(info, k)) for k, _ in info._fields_})
    p.nt, p.drop = bool(p.nt), bool(p.drop)
    return p


def idwt_level_cl_plan(filter_len: int, C: int, d: Sequence[int], t: Sequence[int], has_drop: bool = False,
                       num_cus: int = 0) -> SimpleNamespace:
    """lfgc_idwt_level_cl_plan: the launch idwt_level_cl / idwt_level_cl_drop (has_drop) would make for a level d -> t of
    C channels, nothing enqueued.  num_cus > 0: the z chunking for a device of that many CUs (no device needed); 0: the
    current device's.  Fields: cw, cells, nt, drop, zchunk, nchunks, ptiles, ngroups, threads, lds_bytes, blocks."""
    return _wavelet_cl_plan('lfgc_idwt_level_cl_plan', filter_len, has_drop, C, d, t, num_cus)


def idwt_level_cl_bwd_plan(filter_len: int, C: int, d: Sequence[int], t: Sequence[int], has_drop: bool = False,
                           num_cus: int = 0) -> SimpleNamespace:
    """lfgc_idwt_level_cl_bwd_plan: the same for idwt_level_cl_bwd / idwt_level_cl_drop_bwd (has_drop: factors or L2
    penalties)."""
    return _wavelet_cl_plan('lfgc_idwt_level_cl_bwd_plan', filter_len, has_drop, C, d, t, num_cus)


def _cl_adjoint_groups(L: int, C: int, d: Sequence[int], t: Sequence[int]) -> int:
    """Channel groups of the channel-last adjoint = slices of its deterministic mode: the launch's own selection (it does
    not depend on the CU count or on the DROP build)."""
    return idwt_level_cl_bwd_plan(L, C, d, t, num_cus=1).ngroups


@_on_device
def drop_apply(x: torch.Tensor, mul: torch.Tensor, thr=None) -> torch.Tensor:
    """x (C, ...) * mul (...) with the value rule of include/lfgc.h (one drop layer outside the decode)."""
    _require_hip(x, mul)
    x, mul = _f32c(x), _f32c(mul)
    if tuple(x.shape[1:]) != tuple(mul.shape):
        raise ValueError('drop factor %s does not match coefficients %s' % (tuple(mul.shape), tuple(x.shape)))
    out = torch.empty_like(x)
    check(_lib.load().lfgc_drop_apply_f32(x.data_ptr(), mul.data_ptr(), _thr(thr), out.data_ptr(), x.shape[0],
                                          mul.numel(), _stream(x)), 'lfgc_drop_apply_f32')
    return out


class DropApplyFn(torch.autograd.Function):
    """A drop layer's own forward(x): value by the layer's rule, gradients d_x = g*m, d_m = sum_c g*x."""

    @staticmethod
    @_on_device
    def forward(ctx, x, mul, thr):
        ctx.save_for_backward(x.detach(), mul.detach())
        ctx.need_dm = mul.requires_grad
        return drop_apply(x.detach(), mul.detach(), thr)

    @staticmethod
    @once_differentiable
    @_on_device
    def backward(ctx, g):
        x, mul = ctx.saved_tensors
        g, x, mul = _f32c(g), _f32c(x), _f32c(mul)
        d_x = torch.empty_like(x)
        d_m = torch.empty_like(mul) if ctx.need_dm else None
        check(_lib.load().lfgc_drop_apply_bwd_f32(g.data_ptr(), x.data_ptr(), mul.data_ptr(), d_x.data_ptr(),
                                                  d_m.data_ptr() if d_m is not None else None, x.shape[0], mul.numel(),
                                                  _stream(g)), 'lfgc_drop_apply_bwd_f32')
        return d_x, d_m, None


@_on_device
def decode_levels_drop(coeffs, factors, thresholds, shape_array, filter_rev, channel_last: bool) -> torch.Tensor:
    """decode_volume() with drop factors (model/Feature_Grid_Model.py:102-108): factors[i] / thresholds[i] belong
    to coeffs[i]; None = that tensor passes unchanged.  channel_last: the last level writes the sampler's layout directly
    (a one-level model's last level is also its first: it takes factors[0] as the low band's factor)."""
    n = len(coeffs) - 1            # grids smaller than 6 voxels have no wavelet level at all (dwt_max_level = 0)
    if n == 0:
        restored = coeffs[0] if factors[0] is None else drop_apply(coeffs[0], factors[0], thresholds[0])
        return to_channel_last(restored) if channel_last else restored
    restored, mul_l, thr_l = coeffs[0], factors[0], thresholds[0]
    for k in range(1, n + 1):
        restored = _synthesis(restored, coeffs[k], filter_rev, shape_array[k - 1], mul_l, thr_l, factors[k], thresholds[k],
                              channel_last=channel_last and k == n)
        mul_l, thr_l = None, None
    return restored


def decode_levels(coeffs: Sequence[torch.Tensor], shape_array, filter_rev: torch.Tensor,
                  channel_last: bool) -> torch.Tensor:
    """All IDWT levels (model/Feature_Grid_Model.py:102-108, drop layers already applied by the caller);
    channel_last: the last level writes the sampler's layout directly."""
    none = [None] * len(coeffs)
    return decode_levels_drop(coeffs, none, none, shape_array, filter_rev, channel_last)


def _decode_forward(ctx, filter_rev, shape_array, channel_last, thresholds, coeffs, factors, l1_flags):
    """Context set-up and decode shared by the three decode nodes -> (grid, detached coeffs, detached factors)."""
    n = len(coeffs)
    ctx.filter_rev = filter_rev
    ctx.shape_array = [tuple(int(v) for v in s) for s in shape_array]
    ctx.channel_last = bool(channel_last)
    ctx.n = n
    ctx.dims = [tuple(c.shape) for c in coeffs]
    ctx.want = [f is not None and f.requires_grad for f in factors]
    ctx.has = [f is not None for f in factors]
    ctx.l1_flags = [bool(f) and factors[i] is not None for i, f in enumerate(l1_flags)]
    ctx.deterministic = deterministic_enabled()
    det = [c.detach() for c in coeffs]
    fdet = [f.detach() if f is not None else None for f in factors]
    ctx.save_for_backward(*det, *[f for f in fdet if f is not None])
    with torch.no_grad():
        return decode_levels_drop(det, fdet, list(thresholds), ctx.shape_array, filter_rev, ctx.channel_last), det, fdet


class DecodeVolumeFn(torch.autograd.Function):
    """decode_volume() as one autograd node: IDWT chain forward, adjoint chain backward."""

    @staticmethod
    def forward(ctx, filter_rev, shape_array, channel_last, *coeffs):
        none = [None] * len(coeffs)
        out = _decode_forward(ctx, filter_rev, shape_array, channel_last, none, coeffs, none, none)[0]
        # zero levels and channel-first: the output would alias the parameter; hand autograd a fresh tensor
        return out.clone() if out.data_ptr() == coeffs[0].data_ptr() else out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        return (None, None, None) + tuple(_decode_drop_backward(ctx, d_out, None)[0])


class DecodeVolumeDropFn(torch.autograd.Function):
    """decode_volume() with the drop layers folded into the IDWT kernels, as one autograd node.
    apply(filter_rev, shape_array, channel_last, thresholds, n, *coeffs, *factors) -- n coefficient tensors, then n
    factors (tensor or None); needs at least one wavelet level."""

    @staticmethod
    def forward(ctx, filter_rev, shape_array, channel_last, thresholds, n, *tensors):
        return _decode_forward(ctx, filter_rev, shape_array, channel_last, thresholds, tensors[:n], tensors[n:],
                               [False] * n)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        d_coef, d_fac = _decode_drop_backward(ctx, d_out, None)
        return (None, None, None, None, None) + tuple(d_coef) + tuple(d_fac)


@_on_device
def _decode_drop_backward(ctx, d_out, d_pen):
    """Shared backward of the decode nodes; d_pen fp32 or None = upstream gradients of the penalty sums (layout of
    DecodeVolumePenaltyFn) folded into the adjoint kernels."""
    n = ctx.n
    saved = list(ctx.saved_tensors)
    coeffs = saved[:n]
    it = iter(saved[n:])
    factors = [next(it) if h else None for h in ctx.has]
    C = ctx.dims[0][0]
    # channel_last: the last level's adjoint reads the gradient of the sampler's layout directly
    g = to_channel_first(d_out, C) if (ctx.channel_last and n == 1) else d_out
    d_coef, d_fac = [None] * n, [None] * n
    # the factor gradients are accumulated with atomics: one zero fill for all of them
    sizes = [int(np.prod(ctx.dims[i][1:])) if ctx.want[i] else 0 for i in range(n)]
    flat = torch.zeros(sum(sizes), dtype=torch.float32, device=g.device) if sum(sizes) else None
    zeroed, at = [False] * n, 0
    for i in range(n):
        if sizes[i]:
            zeroed[i] = flat[at:at + sizes[i]].view(ctx.dims[i][1:])
            at += sizes[i]
    if d_pen is not None:
        d_pen = _f32c(d_pen)
        base = d_pen.data_ptr()
        l2 = lambda i: base + 4 * i
        l1 = lambda i: (base + 4 * (n + ctx.l1_pos[i])) if (ctx.l1_flags[i] and zeroed[i] is not False) else 0
    for lvl in range(n - 1, 0, -1):
        first = lvl == 1
        ml = factors[0] if first else None
        pens = None
        if d_pen is not None:
            pens = [l2(0) if first else 0, l2(lvl), l1(0) if first else 0, l1(lvl)]
        lll = coeffs[0] if (first and (ctx.has[0] or d_pen is not None)) else None
        g, d_hf, d_ml, d_mh = _adjoint(g, C, ctx.filter_rev, lll, coeffs[lvl], ml, factors[lvl],
                                       zeroed[0] if first else False, zeroed[lvl], ctx.dims[lvl][2:], pens,
                                       ctx.channel_last and lvl == n - 1, deterministic=ctx.deterministic)
        d_coef[lvl], d_fac[lvl] = d_hf, d_mh
        if first:
            d_fac[0] = d_ml
    d_coef[0] = g
    return d_coef, d_fac


@_on_device
def _penalty_sums(kinds, tensors):
    """All penalty terms in one lfgc_penalty_sums_f32 launch -> fp32 (len(kinds),)."""
    terms, keep = _penalty_terms(kinds, tensors)
    sums = torch.empty(len(kinds) * (1 + _lib.PENALTY_BLOCKS), dtype=torch.float64, device=keep[0][0].device)   # results + scratch
    check(_lib.load().lfgc_penalty_sums_f32(terms, len(kinds), sums.data_ptr(), _stream(sums)), 'lfgc_penalty_sums_f32')
    return sums[:len(kinds)].float()


class DecodeVolumePenaltyFn(torch.autograd.Function):
    """DecodeVolumeDropFn that also returns the penalty sums of its inputs, so that their gradients ride in the adjoint
    kernels instead of costing passes (and autograd accumulation adds) of their own:
    apply(filter_rev, shape_array, channel_last, thresholds, n, l1_flags, *coeffs, *factors) -> (grid, pen) with
    pen fp32 = [sum coeffs[i]^2 for i in range(n)] followed by [sum |factors[i]| for the i with l1_flags[i]] (in order):
    factors that ARE the penalised parameter, e.g. Smallify betas."""

    @staticmethod
    def forward(ctx, filter_rev, shape_array, channel_last, thresholds, n, l1_flags, *tensors):
        ctx.set_materialize_grads(False)
        grid, det, fdet = _decode_forward(ctx, filter_rev, shape_array, channel_last, thresholds, tensors[:n],
                                          tensors[n:], l1_flags)
        l1_idx = [i for i in range(n) if ctx.l1_flags[i]]
        ctx.l1_pos = {i: j for j, i in enumerate(l1_idx)}
        pen = _penalty_sums([_lib.PENALTY_L2] * n + [_lib.PENALTY_L1] * len(l1_idx), det + [fdet[i] for i in l1_idx])
        return grid, pen

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, d_pen):
        if d_out is None:
            raise RuntimeError('the decoded grid took no part in the loss (only its penalties did): unsupported')
        d_coef, d_fac = _decode_drop_backward(ctx, d_out, d_pen)
        return (None, None, None, None, None, None) + tuple(d_coef) + tuple(d_fac)


@_on_device
def sign_variance_update(betas: torch.Tensor, ema: torch.Tensor, emavar: torch.Tensor, momentum: float) -> None:
    """In-place EMA / EMA-variance step of the Smallify sign tracker (model/Smallify_Dropout.py:106-112)."""
    _require_hip(betas, ema, emavar)
    if not (ema.is_contiguous() and emavar.is_contiguous() and ema.dtype == emavar.dtype == torch.float32):
        raise ValueError('tracker state must be contiguous fp32')
    b = _f32c(betas.detach())
    check(_lib.load().lfgc_sign_variance_update_f32(b.data_ptr(), ema.data_ptr(), emavar.data_ptr(), float(momentum),
                                                    b.numel(), _stream(b)), 'lfgc_sign_variance_update_f32')


@_on_device
def sign_variance_update_multi(betas, emas, emavars, momentum: float) -> None:
    """sign_variance_update for all drop layers of a model in one launch."""
    bs = [_f32c(b.detach()) for b in betas]
    _require_hip(*bs, *emas, *emavars)
    for e, v in zip(emas, emavars):
        if not (e.is_contiguous() and v.is_contiguous() and e.dtype == v.dtype == torch.float32):
            raise ValueError('tracker state must be contiguous fp32')
    pb, _k1 = _lib.ptr_array([b.data_ptr() for b in bs])
    pe, _k2 = _lib.ptr_array([e.data_ptr() for e in emas])
    pv, _k3 = _lib.ptr_array([v.data_ptr() for v in emavars])
    ns = (ctypes.c_int64 * len(bs))(*[b.numel() for b in bs])
    check(_lib.load().lfgc_sign_variance_update_multi_f32(pb, pe, pv, ns, len(bs), float(momentum), _stream(bs[0])),
          'lfgc_sign_variance_update_multi_f32')


def _penalty_terms(kinds, tensors):
    if len(kinds) > _lib.PENALTY_MAX_TERMS:
        raise ValueError('at most %d penalty terms per launch' % _lib.PENALTY_MAX_TERMS)
    terms = (_lib.PenaltyTerm * len(kinds))()
    keep, it = [], iter(tensors)
    for t, kind in enumerate(kinds):
        a = _f32c(next(it).detach())
        b = _f32c(next(it).detach()) if kind == _lib.PENALTY_DKL else None
        _require_hip(a, b)
        if b is not None and b.shape != a.shape:
            raise ValueError('log_thetas / log_var shapes differ')
        keep.append((a, b))
        terms[t].a, terms[t].b, terms[t].n, terms[t].kind = a.data_ptr(), (b.data_ptr() if b is not None else None), a.numel(), kind
    return terms, keep


class PenaltyFn(torch.autograd.Function):
    """All penalty terms of a pruning loss in one reduction launch (+ one gradient launch).
    apply(kinds, *tensors) -> fp32 (len(kinds),); a DKL term consumes two tensors (log_thetas, log_var)."""

    @staticmethod
    def forward(ctx, kinds, *tensors):
        ctx.kinds = [int(k) for k in kinds]
        ctx.save_for_backward(*[t.detach() for t in tensors])
        return _penalty_sums(ctx.kinds, tensors)

    @staticmethod
    @once_differentiable
    @_on_device
    def backward(ctx, d_sums):
        tensors = ctx.saved_tensors
        terms, keep = _penalty_terms(ctx.kinds, tensors)
        d_sums = _f32c(d_sums)
        ga = [torch.empty_like(a) for a, _ in keep]
        gb = [torch.empty_like(b) if b is not None else None for _, b in keep]
        pa, _k1 = _lib.ptr_array([g.data_ptr() for g in ga])
        pb, _k2 = _lib.ptr_array([g.data_ptr() if g is not None else 0 for g in gb])
        check(_lib.load().lfgc_penalty_grads_f32(terms, len(ctx.kinds), d_sums.data_ptr(), pa, pb, _stream(d_sums)),
              'lfgc_penalty_grads_f32')
        flat = []
        for g_a, g_b in zip(ga, gb):
            flat.append(g_a)
            if g_b is not None:
                flat.append(g_b)
        return (None,) + tuple(g.view(t.shape) for g, t in zip(flat, tensors))


def penalty_sums(kinds, tensors) -> torch.Tensor:
    return PenaltyFn.apply(list(kinds), *tensors)


# ---- fused sample + embed + MLP ------------------------------------------------------------------------

@_on_device
def pack_mlp(desc: MlpDesc, weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor]) -> torch.Tensor:
    lib = _lib.load()
    ws = [_f32c(w.detach()) for w in weights]
    bs = [_f32c(b.detach()) for b in biases]
    _require_hip(*ws, *bs)
    nbytes = int(lib.lfgc_packed_bytes(ctypes.byref(desc)))
    packed = torch.empty(nbytes // 4, dtype=torch.float32, device=ws[0].device)
    wp, _k1 = _lib.ptr_array([w.data_ptr() for w in ws])
    bp, _k2 = _lib.ptr_array([b.data_ptr() for b in bs])
    check(lib.lfgc_pack_mlp_f32(ctypes.byref(desc), wp, bp, packed.data_ptr(), _stream(packed)), 'lfgc_pack_mlp_f32')
    return packed


def _positions_struct(pos: Optional[torch.Tensor], lattice=None) -> Tuple[Positions, int]:
    ps = Positions()
    if pos is not None:
        ps.pos = pos.data_ptr()
        ps.n = pos.shape[0]
        ps.res[0] = ps.res[1] = ps.res[2] = 2
        ps.x_begin, ps.x_end, ps.tile = 0, 0, 32
        return ps, int(pos.shape[0])
    res, x_begin, x_end, tile = lattice
    ps.pos = None
    ps.n = 0
    for a in range(3):
        ps.res[a] = int(res[a])
    ps.x_begin, ps.x_end, ps.tile = int(x_begin), int(x_end), int(tile)
    return ps, (int(x_end) - int(x_begin)) * int(res[1]) * int(res[2])


@_on_device
def forward_raw(desc: MlpDesc, grid_cl: torch.Tensor, packed: torch.Tensor, pos: Optional[torch.Tensor] = None,
                lattice=None, clamp: bool = False, want_stash: bool = False, out: Optional[torch.Tensor] = None,
                precision: str = 'f16x2', range_fallback: bool = True, return_status: bool = False,
                stash: Optional[torch.Tensor] = None):
    """lfgc_forward_f32.  pos (N,3) or lattice=(res, x_begin, x_end, tile).  Returns (y (N,), stash or None)
    [+ the device status word with return_status].  range_fallback=False returns out-of-range samples of the f16
    builds as NaN instead of redoing the pass on the exact build (diagnostics).  stash: with want_stash, a contiguous fp32
    buffer to write the stash into when it is large enough (a caller that runs chunk after chunk reuses one)."""
    lib = _lib.load()
    _require_hip(grid_cl, packed, pos)
    if pos is not None:
        pos = _f32c(pos)
    ps, n = _positions_struct(pos, lattice)
    D, H, W, cs = grid_cl.shape
    if cs != grid_channel_stride(desc.grid_channels):
        raise ValueError('channel-last grid has stride %d, expected %d' % (cs, grid_channel_stride(desc.grid_channels)))
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=grid_cl.device)
    if n == 0:
        return out, (torch.empty(0, dtype=torch.float32, device=grid_cl.device) if want_stash else None)
    if want_stash:
        floats = int(lib.lfgc_stash_bytes(ctypes.byref(desc), n)) // 4
        if (stash is None or stash.numel() < floats or stash.dtype != torch.float32 or not stash.is_contiguous()
                or stash.device != grid_cl.device):
            stash = torch.empty(floats, dtype=torch.float32, device=grid_cl.device)
    else:
        stash = None
    # range status word of the f16 builds: the library clears it, the kernel sets it, and the exact-fp32 redo the library
    # enqueues behind the kernel is predicated on it -- all in stream order, nothing is read back here
    status = torch.empty(1, dtype=torch.int32, device=grid_cl.device) if (range_fallback and precision != 'fp32') else None
    check(lib.lfgc_forward_f32(ctypes.byref(desc), ctypes.byref(ps), grid_cl.data_ptr(), D, H, W, packed.data_ptr(),
                               _lib.PRECISION[precision], int(clamp), out.data_ptr(),
                               stash.data_ptr() if stash is not None else None,
                               status.data_ptr() if status is not None else None, _stream(grid_cl)), 'lfgc_forward_f32')
    if _DEBUG_STATUS and status is not None:        # diagnostics: LFGC_DEBUG_STATUS=1 (synchronises)
        print('[lfgc] forward n=%d precision=%s status=%d' % (n, precision, int(status.item())), flush=True)
    if return_status:
        return out, stash, status
    return out, stash


def _launch_dict(l: _lib.ForwardLaunch) -> dict:
    return {name: int(getattr(l, name)) for name, _t in _lib.ForwardLaunch._fields_}


@_on_device
def forward_plan(desc: MlpDesc, grid_cl: torch.Tensor, pos: Optional[torch.Tensor] = None, lattice=None,
                 want_stash: bool = False, precision: str = 'f16x2', range_fallback: bool = True) -> SimpleNamespace:
    """lfgc_forward_plan: the launch forward_raw would make for the same arguments on grid_cl's device, nothing enqueued.
    Fields: CH, MT, resident, waves, nbatches, grid, coord_table, zrun, nzc, tiles_per_row, x2, ntiles, lds_bytes (of the
    build `precision` names) and redo = the same fields of the exact-fp32 range-fallback launch, or None without one."""
    _require_hip(grid_cl, pos)
    ps, _n = _positions_struct(pos, lattice)
    D, H, W, _cs = grid_cl.shape
    has_status = range_fallback and precision != 'fp32'
    info = _lib.ForwardPlanInfo()
    check(_lib.load().lfgc_forward_plan(ctypes.byref(desc), ctypes.byref(ps), D, H, W, _lib.PRECISION[precision],
                                        int(want_stash), int(has_status), ctypes.byref(info)), 'lfgc_forward_plan')
    return SimpleNamespace(CH=int(info.CH), MT=int(info.MT), **_launch_dict(info.first),
                           redo=SimpleNamespace(**_launch_dict(info.redo)) if info.has_redo else None)


def backward_plan(desc: MlpDesc, n: int, precision: str = 'f16x2', device=None) -> SimpleNamespace:
    """lfgc_backward_plan: the launch backward_raw would make for n samples on `device` (default: the current one).
    Fields: CH, MT, waves, nbatches, grid, nslabs, roles, lds_bytes."""
    info = _lib.BackwardPlanInfo()
    with torch.cuda.device(device):
        check(_lib.load().lfgc_backward_plan(ctypes.byref(desc), int(n), _lib.PRECISION[precision], ctypes.byref(info)),
              'lfgc_backward_plan')
    return SimpleNamespace(**{name: int(getattr(info, name)) for name, _t in _lib.BackwardPlanInfo._fields_})


@_on_device
def backward_raw(desc: MlpDesc, grid_cl, packed, pos, stash, d_out, weights, biases, need_d_pos: bool,
                 precision: str = 'f16x2', deterministic: bool = False):
    """lfgc_backward_f32 -> (d_grid, d_weights, d_biases, d_pos or None); deterministic: lfgc_backward_det_f32, whose
    d_grid is bitwise independent of the order of the samples (all NaN if any feature gradient is non-finite)."""
    lib = _lib.load()
    pos = _f32c(pos)
    d_out = _f32c(d_out)
    ps, n = _positions_struct(pos)
    D, H, W, cs = grid_cl.shape
    dev = grid_cl.device
    deterministic = bool(deterministic) and n > 0              # an empty batch returns before anything is written
    d_grid = torch.empty_like(grid_cl) if deterministic else torch.zeros_like(grid_cl)   # det: every element is written
    d_w = [torch.empty_like(w, dtype=torch.float32, memory_format=torch.contiguous_format) for w in weights]
    d_b = [torch.empty_like(b, dtype=torch.float32, memory_format=torch.contiguous_format) for b in biases]
    d_pos = torch.empty((n, 3), dtype=torch.float32, device=dev) if need_d_pos else None
    ws_bytes = int(lib.lfgc_backward_det_workspace_bytes(ctypes.byref(desc), n, D, H, W) if deterministic else
                   lib.lfgc_backward_workspace_bytes(ctypes.byref(desc), n))
    if ws_bytes < 0:
        check(ws_bytes, 'lfgc_backward_workspace_bytes')
    ws = torch.empty((max(ws_bytes, 16) + 3) // 4, dtype=torch.float32, device=dev)
    wp, _k1 = _lib.ptr_array([w.data_ptr() for w in d_w])
    bp, _k2 = _lib.ptr_array([b.data_ptr() for b in d_b])
    entry = lib.lfgc_backward_det_f32 if deterministic else lib.lfgc_backward_f32
    check(entry(ctypes.byref(desc), ctypes.byref(ps), grid_cl.data_ptr(), D, H, W, packed.data_ptr(),
                _lib.PRECISION[precision], stash.data_ptr(), d_out.data_ptr(), d_grid.data_ptr(), wp, bp,
                d_pos.data_ptr() if d_pos is not None else None, ws.data_ptr(), ws_bytes,
                _stream(grid_cl)), 'lfgc_backward_det_f32' if deterministic else 'lfgc_backward_f32')
    return d_grid, d_w, d_b, d_pos


def input_gradient_plan(desc: MlpDesc, n: int, precision: str = 'f16x2', device=None) -> SimpleNamespace:
    """lfgc_input_gradient_plan: the launch input_gradient_raw would make for n samples on `device` (default: the current
    one).  Fields as backward_plan's; nslabs and roles are 0 (no weight-gradient kernel follows)."""
    info = _lib.BackwardPlanInfo()
    with torch.cuda.device(device):
        check(_lib.load().lfgc_input_gradient_plan(ctypes.byref(desc), int(n), _lib.PRECISION[precision], ctypes.byref(info)),
              'lfgc_input_gradient_plan')
    return SimpleNamespace(**{name: int(getattr(info, name)) for name, _t in _lib.BackwardPlanInfo._fields_})


@_on_device
def input_gradient_raw(desc: MlpDesc, grid_cl, packed, pos, stash, d_out=None, precision: str = 'f16x2',
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lfgc_input_gradient_f32 -> (N,3) = d_out * d y / d pos (d_out None: ones, the gradient of the unclamped output).
    stash: written by forward_raw(want_stash=True) for the same grid, blob and positions.  out: a contiguous fp32 (N,3)
    tensor (or view) to write into.  Builds no autograd graph, needs no workspace."""
    _require_hip(grid_cl, packed, pos, stash, d_out, out)
    pos = _f32c(pos)
    ps, n = _positions_struct(pos)
    D, H, W, cs = grid_cl.shape
    if cs != grid_channel_stride(desc.grid_channels):
        raise ValueError('channel-last grid has stride %d, expected %d' % (cs, grid_channel_stride(desc.grid_channels)))
    if d_out is not None:
        d_out = _f32c(d_out).reshape(-1)
        if d_out.numel() != n:
            raise ValueError('d_out has %d elements for %d positions' % (d_out.numel(), n))
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=grid_cl.device)
    elif tuple(out.shape) != (n, 3) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError('out must be contiguous fp32 of shape (%d, 3)' % n)
    if n == 0:
        return out
    if stash.numel() * 4 < int(_lib.load().lfgc_stash_bytes(ctypes.byref(desc), n)):
        raise ValueError('stash too small for %d samples' % n)
    check(_lib.load().lfgc_input_gradient_f32(ctypes.byref(desc), ctypes.byref(ps), grid_cl.data_ptr(), D, H, W,
                                              packed.data_ptr(), _lib.PRECISION[precision], stash.data_ptr(), _ptr(d_out),
                                              out.data_ptr(), _stream(grid_cl)), 'lfgc_input_gradient_f32')
    return out


def gradient_chunk_samples(desc: MlpDesc, n: int, max_stash_bytes: int) -> int:
    """Samples per chunk of a value-and-gradient pass over n samples: the largest multiple of 256 whose stash
    (lfgc_stash_bytes: whole 256-sample groups) fits max_stash_bytes -- never below 256 and never beyond n rounded up to
    256.  Host arithmetic only."""
    per_group = int(_lib.load().lfgc_stash_bytes(ctypes.byref(desc), 256))
    groups = max(1, int(max_stash_bytes) // per_group)
    return 256 * max(1, min(groups, (int(n) + 255) // 256))


class SampleDecodeFn(torch.autograd.Function):
    """model/Feature_Grid_Model.py:62-75 as one autograd node (HIP forward + HIP backward)."""

    @staticmethod
    def forward(ctx, desc, pos, grid_cl, packed, n_layers, precision, *params):
        weights, biases = params[:n_layers + 1], params[n_layers + 1:]
        need_grad = any(t.requires_grad for t in (pos, grid_cl) + tuple(params))
        y, stash = forward_raw(desc, grid_cl.detach(), packed, pos=pos.detach(), clamp=False, want_stash=need_grad,
                               precision=precision)
        if need_grad:
            ctx.desc = desc
            ctx.precision = precision
            ctx.n_layers = n_layers
            ctx.need_d_pos = pos.requires_grad
            ctx.deterministic = deterministic_enabled()
            ctx.save_for_backward(pos.detach(), grid_cl.detach(), packed, stash, *[p.detach() for p in params])
        return y.view(-1, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_y):
        pos, grid_cl, packed, stash = ctx.saved_tensors[:4]
        params = ctx.saved_tensors[4:]
        L = ctx.n_layers
        weights, biases = params[:L + 1], params[L + 1:]
        d_grid, d_w, d_b, d_pos = backward_raw(ctx.desc, grid_cl, packed, pos, stash, d_y.reshape(-1), weights, biases,
                                               ctx.need_d_pos, precision=ctx.precision, deterministic=ctx.deterministic)
        return (None, d_pos, d_grid, None, None, None) + tuple(d_w) + tuple(d_b)


# ---- binary checkpoint codec, device side -------------------------------------------

def _flat_f32(x: torch.Tensor) -> torch.Tensor:
    _require_hip(x)
    return _f32c(x.detach()).reshape(-1)


def _select_workspace(n: int, device, query: str = 'lfgc_codec_select_workspace_bytes') -> torch.Tensor:
    """Scratch of one order-preserving selection over n elements (csrc/lfgc_select.h), sized by the entry's own query."""
    nbytes = int(getattr(_lib.load(), query)(int(n)))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)


@_on_device
def codec_mask(x: torch.Tensor) -> torch.Tensor:
    """uint8 (ceil(n/8),): bit i (MSB first) = x.flat[i] != 0."""
    x = _flat_f32(x)
    mask = torch.empty((x.numel() + 7) // 8, dtype=torch.uint8, device=x.device)
    check(_lib.load().lfgc_codec_mask_f32(x.data_ptr(), x.numel(), mask.data_ptr(), _stream(x)), 'lfgc_codec_mask_f32')
    return mask


@_on_device
def codec_compact(x: torch.Tensor) -> torch.Tensor:
    """The non-zero values of x in order (1-D).  Synchronises once to learn their number."""
    x = _flat_f32(x)
    out = torch.empty_like(x)
    count = torch.zeros(1, dtype=torch.int64, device=x.device)
    ws = _select_workspace(x.numel(), x.device)
    check(_lib.load().lfgc_codec_compact_f32(x.data_ptr(), x.numel(), out.data_ptr(), count.data_ptr(), ws.data_ptr(),
                                             ws.numel() * 8, _stream(x)), 'lfgc_codec_compact_f32')
    return out[:int(count.item())]


_SELECT_PER_BLOCK = 2048          # kSelectPerBlock of csrc/lfgc_select.h: elements per workgroup of a selection


@_on_device
def codec_expand(mask: torch.Tensor, bit_offset: int, n: int, values: torch.Tensor, counted: bool = False):
    """(n,) fp32: values scattered to the set bits [bit_offset, bit_offset + n) of the MSB-first mask, zeros elsewhere.
    ``counted``: (that, the number of set bits in the range as a 0-d device int64 -- the selection's scanned total, which
    stays in its workspace behind the block offsets; no synchronisation)."""
    out, ws = _codec_expand(mask, bit_offset, n, values)
    return (out, ws[-(-int(n) // _SELECT_PER_BLOCK)]) if counted else out


def _codec_expand(mask, bit_offset, n, values):
    _require_hip(mask, values)
    if mask.dtype != torch.uint8 or (int(bit_offset) + int(n) + 7) // 8 > mask.numel():
        raise ValueError('mask too short for %d bits at offset %d' % (n, bit_offset))
    values = _f32c(values).reshape(-1)
    if values.numel() == 0:
        values = torch.zeros(1, dtype=torch.float32, device=mask.device)
    out = torch.empty(int(n), dtype=torch.float32, device=mask.device)
    ws = _select_workspace(n, mask.device)
    check(_lib.load().lfgc_codec_expand_f32(mask.contiguous().data_ptr(), int(bit_offset), int(n), values.data_ptr(),
                                            out.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(mask)), 'lfgc_codec_expand_f32')
    return out, ws


# ---- the mask once per cell: support + residual (mode 2 of the mask file; csrc/lfgc_chanmask.hip) --------------

def _cells(x: torch.Tensor, C: int) -> Tuple[torch.Tensor, int, int]:
    C = int(C)
    if C < 1 or x.numel() < 1 or x.numel() % C:
        raise ValueError('a tensor of %d coefficients is no whole number (at least one) of cells of %d channels' % (x.numel(), C))
    return _flat_f32(x), C, x.numel() // C


@_on_device
def codec_support(x: torch.Tensor, C: int) -> torch.Tensor:
    """uint8 (S,): 1 where any of the C channels of cell j is non-zero, x viewed as (C, S) in its flat order."""
    x, C, S = _cells(x, C)
    flags = torch.empty(S, dtype=torch.uint8, device=x.device)
    check(_lib.load().lfgc_codec_support_f32(x.data_ptr(), C, S, flags.data_ptr(), _stream(x)), 'lfgc_codec_support_f32')
    return flags


@_on_device
def codec_pack_flags(flags: torch.Tensor) -> torch.Tensor:
    """uint8 (ceil(n/8),): bit i (MSB first) = flags.flat[i] != 0 of a uint8 tensor, tail bits zero."""
    flags = _flat_u8(flags, 'flags')
    _require_hip(flags)
    if flags.numel() < 1:
        raise ValueError('flag packing needs at least one flag')
    bits = torch.empty((flags.numel() + 7) // 8, dtype=torch.uint8, device=flags.device)
    check(_lib.load().lfgc_codec_pack_flags_u8(flags.data_ptr(), flags.numel(), bits.data_ptr(), _stream(flags)),
          'lfgc_codec_pack_flags_u8')
    return bits


@_on_device
def codec_compact_support(x: torch.Tensor, C: int, flags: torch.Tensor) -> torch.Tensor:
    """(C, K) fp32: the cells of x (viewed as (C, S)) whose flag is set, in order.  Synchronises once to learn K."""
    x, C, S = _cells(x, C)
    flags = _flat_u8(flags, 'flags')
    _require_hip(flags)
    if flags.numel() != S:
        raise ValueError('%d flags for %d cells' % (flags.numel(), S))
    V = torch.empty(C * S, dtype=torch.float32, device=x.device)
    count = torch.zeros(1, dtype=torch.int64, device=x.device)
    ws = _select_workspace(S, x.device)
    check(_lib.load().lfgc_codec_compact_support_f32(x.data_ptr(), C, S, flags.data_ptr(), V.data_ptr(), count.data_ptr(),
                                                     ws.data_ptr(), ws.numel() * 8, _stream(x)), 'lfgc_codec_compact_support_f32')
    K = int(count.item())
    return V[:C * K].view(C, K)


@_on_device
def codec_expand_support(support: torch.Tensor, bit_offset: int, C: int, S: int, V: torch.Tensor, K: int,
                         status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(C * S,) fp32: cell j of every channel c is V[c * K + rank] where bit (bit_offset + j) of the MSB-first support stream
    is set, zero elsewhere.  K is the caller's word for the number of set bits: the kernel clamps every index into V to
    C * K - 1 and sets bit 0 of ``status`` (device int32, one element, accumulated over calls, no synchronisation) where the
    support holds another number.  Without ``status`` the wrapper checks it itself, synchronising, and raises ValueError."""
    _require_hip(support, V, status)
    bit_offset, C, S, K = int(bit_offset), int(C), int(S), int(K)
    if C < 1 or S < 1 or bit_offset < 0 or not 0 <= K <= S:
        raise ValueError('expansion needs C >= 1, S >= 1, a bit offset >= 0 and 0 <= K <= S, got C = %d, S = %d, offset %d, '
                         'K = %d' % (C, S, bit_offset, K))
    if support.dtype != torch.uint8 or (bit_offset + S + 7) // 8 > support.numel():
        raise ValueError('support too short for %d bits at offset %d' % (S, bit_offset))
    V = _f32c(V).reshape(-1)
    if V.numel() < C * K:
        raise ValueError('%d values where C * K = %d are needed' % (V.numel(), C * K))
    if V.numel() == 0:
        V = torch.zeros(1, dtype=torch.float32, device=support.device)
    own = status is None
    if own:
        status = torch.zeros(1, dtype=torch.int32, device=support.device)
    elif status.dtype != torch.int32 or status.numel() != 1 or not status.is_contiguous():
        raise ValueError('status must be one int32')
    out = torch.empty(C * S, dtype=torch.float32, device=support.device)
    ws = _select_workspace(S, support.device)
    check(_lib.load().lfgc_codec_expand_support_f32(support.contiguous().data_ptr(), bit_offset, C, S, V.data_ptr(), K,
                                                    out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                                    _stream(support)), 'lfgc_codec_expand_support_f32')
    if own and int(status.item()):
        raise ValueError('the support holds a number of set bits other than K = %d' % K)
    return out


def _ward_init(sample: torch.Tensor, k: int, device) -> torch.Tensor:
    """(k,) fp32 sorted initial centres on `device` from a SORTED sample (host C++, lfgc_codec_ward_init_host)."""
    sample = np.ascontiguousarray(sample.cpu().numpy())
    init = np.empty(k, dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    check(_lib.load().lfgc_codec_ward_init_host(sample.ctypes.data_as(fp), sample.size, int(k), init.ctypes.data_as(fp)),
          'lfgc_codec_ward_init_host')
    return torch.from_numpy(init).to(device)


@_on_device
def codec_kmeans_sorted(x_sorted: torch.Tensor, init: torch.Tensor, iterations: int = 40) -> torch.Tensor:
    """(k,) fp32 sorted centres after `iterations` Lloyd steps over the ASCENDING values x_sorted, from the sorted initial
    centres `init` (k <= 65 536; lfgc_codec_kmeans1d_sorted_f32)."""
    xs = _flat_f32(x_sorted)
    _require_hip(init)
    centres = _f32c(init.detach()).reshape(-1).clone()
    n, k = xs.numel(), centres.numel()
    lib = _lib.load()
    if n < 1 or not 1 <= k <= 65536:
        raise ValueError('k-means needs at least one value and 1 <= k <= 65536')
    nbytes = int(lib.lfgc_codec_kmeans_sorted_workspace_bytes(n, k))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=xs.device)
    check(lib.lfgc_codec_kmeans1d_sorted_f32(xs.data_ptr(), n, k, centres.data_ptr(), int(iterations), ws.data_ptr(),
                                             ws.numel() * 8, _stream(xs)), 'lfgc_codec_kmeans1d_sorted_f32')
    return centres


@_on_device
def codec_labels_u16(x: torch.Tensor, centres: torch.Tensor) -> torch.Tensor:
    """(n,) uint16: index of the nearest of the sorted `centres` (k <= 65 536) for every value of x, by the k-means entries'
    own rule (number of fp32 midpoints < value)."""
    x = _flat_f32(x)
    _require_hip(centres)
    centres = _f32c(centres.detach()).reshape(-1)
    if x.numel() < 1 or not 1 <= centres.numel() <= 65536:
        raise ValueError('labels need at least one value and 1 <= k <= 65536')
    labels = torch.empty(x.numel(), dtype=torch.uint16, device=x.device)
    check(_lib.load().lfgc_codec_labels_u16_f32(x.data_ptr(), x.numel(), centres.numel(), centres.data_ptr(),
                                                labels.data_ptr(), _stream(x)), 'lfgc_codec_labels_u16_f32')
    return labels


@_on_device
def codec_kmeans(x: torch.Tensor, k: int = 256, iterations: int = 40) -> Tuple[torch.Tensor, torch.Tensor]:
    """(centres (k,) fp32 sorted, labels (n,): uint8 for k <= 256, uint16 above) of the 1-D value set x, 1 <= k <= 65 536.
    Initial centres: Ward merging (host C++, lfgc_codec_ward_init_host) of a sorted strided sample; then Lloyd iterations
    over all values on the GPU.  k <= 256: a sample of at most 2^16 values and lfgc_codec_kmeans1d_f32 (LDS histograms).
    k > 256: the values are sorted once, the sample is every stride-th of them -- min(n, max(2^16, 16 k)) values, at most
    2^20 -- and lfgc_codec_kmeans1d_sorted_f32 + lfgc_codec_labels_u16_f32 do the rest.  (16 k alone starves the tails: a
    12 500-value sample of 50 000 Laplace values gave a 1 024-entry codebook 3.5 times the error of scikit-learn's.)"""
    x = _flat_f32(x)
    n = x.numel()
    if n < 1 or not 1 <= k <= 65536:
        raise ValueError('k-means needs at least one value and 1 <= k <= 65536')
    if k > 256:
        xs = torch.sort(x)[0]
        stride = max(1, -(-n // min(max(1 << 16, 16 * int(k)), 1 << 20)))
        centres = codec_kmeans_sorted(xs, _ward_init(xs[::stride], int(k), x.device), iterations)
        return centres, codec_labels_u16(x, centres)
    lib = _lib.load()
    stride = max(1, -(-n // (1 << 16)))
    centres = _ward_init(torch.sort(x[::stride])[0], int(k), x.device)
    labels = torch.empty(n, dtype=torch.uint8, device=x.device)
    nbytes = int(lib.lfgc_codec_kmeans_workspace_bytes(int(k)))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=x.device)
    check(lib.lfgc_codec_kmeans1d_f32(x.data_ptr(), n, int(k), centres.data_ptr(), labels.data_ptr(), int(iterations),
                                      ws.data_ptr(), ws.numel() * 8, _stream(x)), 'lfgc_codec_kmeans1d_f32')
    return centres, labels


@_on_device
def codec_pack_labels(labels: torch.Tensor, bits: int) -> torch.Tensor:
    """uint8 (ceil(n * bits / 8),): the labels (uint8, or uint16 -- required above 8 bits), `bits` wide each, MSB first; the
    unused low bits of the last byte are zero."""
    _require_hip(labels)
    if labels.dtype not in (torch.uint8, torch.uint16):
        raise ValueError('labels must be uint8 or uint16')
    labels = labels.contiguous().reshape(-1)
    n, bits = labels.numel(), int(bits)
    if n < 1 or not 1 <= bits <= 16 or (bits > 8 and labels.dtype != torch.uint16):
        raise ValueError('label packing needs at least one label, 1 <= bits <= 16 and uint16 labels above 8 bits')
    packed = torch.empty((n * bits + 7) // 8, dtype=torch.uint8, device=labels.device)
    check(_lib.load().lfgc_codec_pack_labels(labels.data_ptr(), labels.element_size(), n, bits, packed.data_ptr(),
                                             packed.numel(), _stream(labels)), 'lfgc_codec_pack_labels')
    return packed


@_on_device
def codec_dequant(packed: torch.Tensor, bits: int, n: int, centres: torch.Tensor) -> torch.Tensor:
    """(n,) fp32 = centres[label_i], labels `bits` wide, MSB first, in the uint8 stream `packed`."""
    _require_hip(packed, centres)
    if packed.dtype != torch.uint8:
        raise ValueError('packed labels must be uint8')
    centres = _f32c(centres)
    if centres.numel() < (1 << int(bits)):
        raise ValueError('codebook smaller than 2^bits')
    out = torch.empty(int(n), dtype=torch.float32, device=packed.device)
    check(_lib.load().lfgc_codec_dequant_f32(packed.contiguous().data_ptr(), packed.numel(), int(bits), int(n),
                                             centres.data_ptr(), out.data_ptr(), _stream(packed)), 'lfgc_codec_dequant_f32')
    return out


# ---- entropy stage of the codec: 64-lane interleaved rANS (include/lfgc.h) ---------------------------------

RANS_ROUNDS = 512                 # rounds per chunk the file writer uses: chunks of 32 768 symbols
RANS_HEADER_BYTES = 8 + 2 * 256   # u32 n | u16 R | u16 0 | u16 f[256]


def codec_rans_header(buf, offset: int = 0, length: Optional[int] = None, exact: bool = False) -> SimpleNamespace:
    """Read and check the header of the rANS stream at buf[offset:] on the HOST (buf: bytes-like; nothing touches the GPU):
    n, rounds, freq (256 int64), words (nc int64), nbytes = 520 + 260 nc + 2 sum(words).  `length` is the number of bytes the
    stream may take from `offset` (default: the rest of buf; buf itself only has to hold the header and the word counts);
    `exact` wants nbytes == length.  ValueError for a truncated stream, rounds < 1, sum f != 4096 or word counts that do
    not fit the length."""
    view = memoryview(buf).cast('B')
    have = len(view) - int(offset)
    length = have if length is None else int(length)
    if offset < 0 or min(have, length) < RANS_HEADER_BYTES:
        raise ValueError('truncated rANS stream: no room for its %d-byte header' % RANS_HEADER_BYTES)
    n, rounds, zero = struct.unpack_from('<IHH', view, offset)
    freq = np.frombuffer(view, '<u2', 256, offset + 8).astype(np.int64)
    if rounds < 1 or zero != 0:
        raise ValueError('rANS stream header: rounds per chunk %d, reserved field %d' % (rounds, zero))
    if int(freq.sum()) != 4096:
        raise ValueError('rANS stream header: the frequencies sum to %d, not 4096' % int(freq.sum()))
    nc = -(-n // (64 * rounds))
    if min(have, length) < RANS_HEADER_BYTES + 4 * nc:
        raise ValueError('truncated rANS stream: %d chunks of %d symbols need %d bytes of word counts' % (nc, 64 * rounds, 4 * nc))
    words = np.frombuffer(view, '<u4', nc, offset + RANS_HEADER_BYTES).astype(np.int64)
    nbytes = RANS_HEADER_BYTES + 260 * nc + 2 * int(words.sum())
    if nbytes > length or (exact and nbytes != length):
        raise ValueError('rANS stream: header, %d chunks and %d words make %d bytes, %d are there'
                         % (nc, int(words.sum()), nbytes, length))
    return SimpleNamespace(n=n, rounds=rounds, freq=freq, words=words, nbytes=nbytes)


def rans_normalize(counts) -> np.ndarray:
    """256 uint16 frequencies summing to 4096 from 256 symbol counts (host C++, lfgc_codec_rans_normalize_host)."""
    counts = np.ascontiguousarray(np.asarray(counts).reshape(-1), dtype=np.int64)
    if counts.size != 256:
        raise ValueError('the model is over byte symbols: 256 counts, got %d' % counts.size)
    freq = np.zeros(256, dtype=np.uint16)
    check(_lib.load().lfgc_codec_rans_normalize_host(counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                     freq.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))),
          'lfgc_codec_rans_normalize_host')
    return freq


def _flat_u8(t: torch.Tensor, what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.uint8:
        raise ValueError('%s must be a uint8 tensor' % what)
    return t.detach().contiguous().reshape(-1)


@_on_device
def codec_histogram_u8(sym: torch.Tensor) -> torch.Tensor:
    """(256,) int64 on the device: how often each byte value occurs in the uint8 tensor."""
    sym = _flat_u8(sym, 'symbols')
    _require_hip(sym)
    counts = torch.zeros(256, dtype=torch.int64, device=sym.device)
    check(_lib.load().lfgc_codec_histogram_u8(sym.data_ptr(), sym.numel(), counts.data_ptr(), _stream(sym)),
          'lfgc_codec_histogram_u8')
    return counts


def _rans_workspace(n: int, rounds: int, device) -> torch.Tensor:
    nbytes = int(_lib.load().lfgc_codec_rans_workspace_bytes(int(n), int(rounds)))
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)


@_on_device
def codec_rans_encode(sym_u8: torch.Tensor, rounds: int = RANS_ROUNDS) -> torch.Tensor:
    """The whole rANS stream (device uint8) of a device uint8 tensor of 1 to 2^32 - 1 symbols, `rounds` (1 to 65 535) rounds
    per chunk.  Synchronises twice: the counts go to the host for the normalisation, and the number of words sizes the
    stream."""
    sym = _flat_u8(sym_u8, 'symbols')
    _require_hip(sym)
    n, rounds = sym.numel(), int(rounds)
    if not 1 <= n < 1 << 32 or not 1 <= rounds <= 0xFFFF:
        raise ValueError('rANS codes 1 to 2^32 - 1 symbols in chunks of 1 to 65535 rounds, got n = %d, rounds = %d' % (n, rounds))
    lib = _lib.load()
    freq = torch.from_numpy(rans_normalize(codec_histogram_u8(sym).cpu().numpy()).view(np.int16)).to(sym.device)
    ws = _rans_workspace(n, rounds, sym.device)
    total = torch.zeros(1, dtype=torch.int64, device=sym.device)
    check(lib.lfgc_codec_rans_encode_count(sym.data_ptr(), n, rounds, freq.data_ptr(), total.data_ptr(), ws.data_ptr(),
                                           ws.numel() * 8, _stream(sym)), 'lfgc_codec_rans_encode_count')
    nc = -(-n // (64 * rounds))
    out = torch.empty(RANS_HEADER_BYTES + 260 * nc + 2 * int(total.item()), dtype=torch.uint8, device=sym.device)
    check(lib.lfgc_codec_rans_encode_write(sym.data_ptr(), n, rounds, freq.data_ptr(), out.data_ptr(), out.numel(),
                                           ws.data_ptr(), ws.numel() * 8, _stream(sym)), 'lfgc_codec_rans_encode_write')
    return out


def codec_rans_decode_parsed(stream: torch.Tensor, info: SimpleNamespace) -> torch.Tensor:
    """The kernel side of codec_rans_decode for a device stream whose header `info` the host has checked."""
    out = torch.empty(info.n, dtype=torch.uint8, device=stream.device)
    if info.n == 0:
        return out
    if stream.data_ptr() % 4:
        stream = stream.clone()
    status = torch.zeros(1, dtype=torch.int32, device=stream.device)
    ws = _rans_workspace(info.n, info.rounds, stream.device)
    check(_lib.load().lfgc_codec_rans_decode(stream.data_ptr(), stream.numel(), info.n, info.rounds, out.data_ptr(),
                                             status.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(stream)),
          'lfgc_codec_rans_decode')
    code = int(status.item())
    if code:
        raise ValueError('malformed rANS stream (status %d: 1 = a lane wanted a word beyond its chunk, 2 = a final state is not '
                         '2^16, 4 = a chunk\'s words were not used up, 8 = a chunk lies outside the stream)' % code)
    return out


@_on_device
def codec_rans_decode(stream_u8: torch.Tensor) -> torch.Tensor:
    """The symbols (device uint8) of a whole rANS stream held in a uint8 tensor.  The header is read and checked on the host
    first (codec_rans_header, exact length); ValueError for a header that fails and for a stream the kernel reports as
    malformed.  Synchronises to read the header and the status word."""
    stream = _flat_u8(stream_u8, 'the stream')
    if stream.is_cuda:                      # the header and the word counts are all the host needs
        head = stream[:RANS_HEADER_BYTES].cpu().numpy().tobytes()
        if len(head) == RANS_HEADER_BYTES:
            n, rounds = int(np.frombuffer(head, '<u4', 1)[0]), int(np.frombuffer(head, '<u2', 1, 4)[0])
            if rounds >= 1:
                nc = -(-n // (64 * rounds))
                head += stream[RANS_HEADER_BYTES:RANS_HEADER_BYTES + 4 * nc].cpu().numpy().tobytes()
    else:
        head = stream.numpy().tobytes()
    info = codec_rans_header(head, 0, stream.numel(), exact=True)
    _require_hip(stream)
    return codec_rans_decode_parsed(stream, info)


# ---- error-bounded residual layer (include/lfgc.h; csrc/lfgc_residual.hip) ----------------------------------

RESIDUAL_ESCAPE = 255             # the symbol of a voxel stored verbatim


def residual_eps(max_error) -> float:
    """float32(max_error) as a Python float.  ValueError unless it, step = eps + eps and 1 / step are positive, normal, finite
    fp32 numbers -- the rule of the C entries, applied on the host."""
    try:
        with np.errstate(all='ignore'):
            eps = np.float32(max_error)
            step = np.float32(eps + eps)
            inv = np.float32(1.0) / step if step != 0 else np.float32(np.inf)
    except (TypeError, ValueError):
        raise ValueError('max_error must be a number, got %r' % (max_error,)) from None
    tiny = np.finfo(np.float32).tiny
    if eps.shape != () or not all(np.isfinite(v) and v >= tiny for v in (eps, step, inv)):
        raise ValueError('max_error, twice it and the reciprocal of that must be positive normal fp32 numbers, got %r' % (max_error,))
    return float(eps)


def _residual_f32(t, what: str, n: Optional[int] = None) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError('%s must be a contiguous float32 tensor' % what)
    if n is not None and t.numel() != n:
        raise ValueError('%s has %d elements where %d are needed' % (what, t.numel(), n))
    return t.detach().reshape(-1)


def _residual_word(t, dtype, what: str, device) -> torch.Tensor:
    """A one-element accumulator of the entries (checksum, status): the caller's, or a zeroed one."""
    if t is None:
        return torch.zeros(1, dtype=dtype, device=device)
    if not torch.is_tensor(t) or t.dtype != dtype or t.numel() != 1 or not t.is_contiguous():
        raise ValueError('%s must be one %s' % (what, str(dtype).replace('torch.', '')))
    return t


@_on_device
def residual_quantize(pred: torch.Tensor, gt: torch.Tensor, max_error, sym: Optional[torch.Tensor] = None,
                      checksum: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(symbols uint8 (n,), checksum int64 (1,)) of a prediction against its ground truth under the bound ``max_error``: 0 to
    254 = the zigzag of the residual in steps of twice the bound, 255 = the voxel is stored verbatim.  The checksum of
    ``pred`` (the uint64 of include/lfgc.h held in an int64) is ADDED to ``checksum`` where one is given.  No synchronisation."""
    eps = residual_eps(max_error)
    p = _residual_f32(pred, 'pred')
    g = _residual_f32(gt, 'gt', p.numel())
    _require_hip(p, g, sym, checksum)
    if p.numel() < 1:
        raise ValueError('the residual layer needs at least one voxel')
    if sym is None:
        sym = torch.empty(p.numel(), dtype=torch.uint8, device=p.device)
    elif sym.dtype != torch.uint8 or sym.numel() != p.numel() or not sym.is_contiguous():
        raise ValueError('sym must be a contiguous uint8 tensor of %d elements' % p.numel())
    checksum = _residual_word(checksum, torch.int64, 'checksum', p.device)
    check(_lib.load().lfgc_residual_quantize_f32(p.data_ptr(), g.data_ptr(), p.numel(), eps, sym.data_ptr(), checksum.data_ptr(),
                                                 _stream(p)), 'lfgc_residual_quantize_f32')
    return sym.reshape(-1), checksum


@_on_device
def residual_outliers(sym: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """The ground truth of the voxels whose symbol is 255, in order, bit for bit (1-D fp32).  Synchronises once to learn
    their number."""
    sym = _flat_u8(sym, 'sym')
    g = _residual_f32(gt, 'gt', sym.numel())
    _require_hip(sym, g)
    if sym.numel() < 1:
        raise ValueError('the residual layer needs at least one voxel')
    out = torch.empty(sym.numel(), dtype=torch.float32, device=sym.device)
    count = torch.zeros(1, dtype=torch.int64, device=sym.device)
    ws = _select_workspace(sym.numel(), sym.device, 'lfgc_residual_workspace_bytes')
    check(_lib.load().lfgc_residual_outliers_f32(sym.data_ptr(), g.data_ptr(), sym.numel(), out.data_ptr(), count.data_ptr(),
                                                 ws.data_ptr(), ws.numel() * 8, _stream(sym)), 'lfgc_residual_outliers_f32')
    return out[:int(count.item())]


@_on_device
def residual_apply(pred: torch.Tensor, sym: torch.Tensor, max_error, outliers: torch.Tensor, out: Optional[torch.Tensor] = None,
                   checksum: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None):
    """(out, checksum int64 (1,), n_escape int64 (1,), status int32 (1,)): the volume restored from a prediction, its symbols
    and the K = ``outliers.numel()`` voxels stored verbatim.  ``out`` may be ``pred`` (default: a new tensor of its shape).
    The kernel never reads past the K outliers: an escape beyond them becomes 0 and sets bit 1 of ``status``, and bit 0 is
    set where the symbols hold another number of escapes than K (``n_escape``: how many).  ``checksum`` and ``status`` are
    accumulated into where given.  No synchronisation: the caller reads the three words when it wants them."""
    eps = residual_eps(max_error)
    p = _residual_f32(pred, 'pred')
    sym = _flat_u8(sym, 'sym')
    if sym.numel() != p.numel():
        raise ValueError('%d symbols for %d voxels' % (sym.numel(), p.numel()))
    if p.numel() < 1:
        raise ValueError('the residual layer needs at least one voxel')
    v = _residual_f32(outliers, 'outliers')
    if v.numel() > p.numel():
        raise ValueError('%d outliers for %d voxels' % (v.numel(), p.numel()))
    _require_hip(p, sym, v, out, checksum, status)
    o = torch.empty_like(pred) if out is None else out
    _residual_f32(o, 'out', p.numel())
    checksum = _residual_word(checksum, torch.int64, 'checksum', p.device)
    status = _residual_word(status, torch.int32, 'status', p.device)
    n_escape = torch.zeros(1, dtype=torch.int64, device=p.device)
    ws = _select_workspace(p.numel(), p.device, 'lfgc_residual_workspace_bytes')
    check(_lib.load().lfgc_residual_apply_f32(p.data_ptr(), sym.data_ptr(), p.numel(), eps, v.data_ptr() if v.numel() else None,
                                              v.numel(), o.data_ptr(), checksum.data_ptr(), n_escape.data_ptr(), status.data_ptr(),
                                              ws.data_ptr(), ws.numel() * 8, _stream(p)), 'lfgc_residual_apply_f32')
    return o, checksum, n_escape, status


# ---- ground truth / statistics -------------------------------------------------------------------------

def _float3(v):
    """Host sequence, array or tensor of 3 numbers -> ctypes float[3]."""
    return (ctypes.c_float * 3)(*[float(x) for x in (v.tolist() if hasattr(v, 'tolist') else v)])


@_on_device
def gt_interp(p: torch.Tensor, f: torch.Tensor, min_bb, max_bb, res) -> torch.Tensor:
    lib = _lib.load()
    _require_hip(p, f)
    p, f = _f32c(p), _f32c(f)
    out = torch.empty(p.shape[0], dtype=torch.float32, device=p.device)
    if p.shape[0] == 0:                 # an empty tensor has no address to hand down (the entry refuses NULL before it reads n)
        return out
    X, Y, Z = f.shape
    check(lib.lfgc_gt_interp_f32(p.data_ptr(), f.data_ptr(), _float3(min_bb), _float3(max_bb), _float3(res), p.shape[0], X, Y, Z,
                                 out.data_ptr(), _stream(p)), 'lfgc_gt_interp_f32')
    return out


class GtMseLossFn(torch.autograd.Function):
    """loss = MSELoss()(pred, trilinear_f_interpolation(p, f, ...)) as one node: ground truth, squared error and the
    gradient of the mean in one kernel (+ a one-workgroup fold).  apply(pred (N,), p (N,3), f (X,Y,Z), min_bb, max_bb, res)
    with the three bounds as host sequences of 3 floats."""

    @staticmethod
    @_on_device
    def forward(ctx, pred, p, f, min_bb, max_bb, res):
        lib = _lib.load()
        _require_hip(pred, p, f)
        pred_c, p, f = _f32c(pred.detach()).reshape(-1), _f32c(p.detach()), _f32c(f.detach())
        n = pred_c.numel()
        if p.shape != (n, 3):
            raise ValueError('positions %s do not match %d predictions' % (tuple(p.shape), n))
        d_pred = torch.empty_like(pred_c)
        loss = torch.empty((), dtype=torch.float32, device=pred_c.device)
        ws = torch.empty(int(lib.lfgc_gt_mse_workspace_bytes(n)) // 8, dtype=torch.float64, device=pred_c.device)
        X, Y, Z = f.shape
        check(lib.lfgc_gt_mse_f32(p.data_ptr(), f.data_ptr(), _float3(min_bb), _float3(max_bb), _float3(res), n, X, Y, Z,
                                  pred_c.data_ptr(), None, d_pred.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                                  ws.numel() * 8, _stream(pred_c)), 'lfgc_gt_mse_f32')
        ctx.save_for_backward(d_pred)
        ctx.shape = pred.shape
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (d_pred,) = ctx.saved_tensors
        unit = _UNIT_GRADS.get(g.device)
        if unit is not None and g.data_ptr() == unit.data_ptr():      # unit_grad(): known to be 1.0
            return d_pred.view(ctx.shape), None, None, None, None, None
        return (d_pred * g).view(ctx.shape), None, None, None, None, None


def gt_mse_loss(pred, p, f, min_bb, max_bb, res) -> torch.Tensor:
    return GtMseLossFn.apply(pred, p, f, min_bb, max_bb, res)


@_on_device
def lattice_positions(flat: torch.Tensor, res, min_idx, max_idx, scales) -> Tuple[torch.Tensor, torch.Tensor]:
    """(raw (N,3), norm (N,3)) for flat voxel indices on the device: lfgc_lattice_positions_f32."""
    _require_hip(flat)
    flat = flat.to(torch.int64).contiguous()
    n = flat.numel()
    raw = torch.empty((n, 3), dtype=torch.float32, device=flat.device)
    norm = torch.empty((n, 3), dtype=torch.float32, device=flat.device)
    if n == 0:
        return raw, norm
    r3 = (ctypes.c_int32 * 3)(*[int(x) for x in res])
    check(_lib.load().lfgc_lattice_positions_f32(flat.data_ptr(), n, r3, _float3(min_idx), _float3(max_idx), _float3(scales),
                                                 raw.data_ptr(), norm.data_ptr(), _stream(flat)), 'lfgc_lattice_positions_f32')
    return raw, norm


def lattice_slab_positions(res, x_begin: int, x_end: int, tile: int, scales, device) -> torch.Tensor:
    """((x_end - x_begin) * Y * Z, 3) normalised positions of the x-slab [x_begin, x_end) of the volume lattice, row-major
    (x, y, z): lfgc_lattice_slab_positions_f32, the positions the fused forward forms for itself in lattice mode."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.LfgcError('the slab positions are formed on the MI355X only: got device %s; there is no CPU fallback.' % device)
    n = (int(x_end) - int(x_begin)) * int(res[1]) * int(res[2])
    with torch.cuda.device(device):
        out = torch.empty((max(n, 0), 3), dtype=torch.float32, device=device)
        r3 = (ctypes.c_int32 * 3)(*[int(x) for x in res])
        check(_lib.load().lfgc_lattice_slab_positions_f32(r3, int(x_begin), int(x_end), int(tile), _float3(scales),
                                                          out.data_ptr(), _stream(out)), 'lfgc_lattice_slab_positions_f32')
    return out


@_on_device
def lattice_sample(state: torch.Tensor, n: int, seed: int, res, min_idx, max_idx, scales,
                   want_flat: bool = False):
    """(raw (N,3), norm (N,3)[, flat (N) int64]) for N voxel indices drawn uniformly (with replacement) by the kernel
    itself: lfgc_lattice_sample_f32.  `state`: device int64[2], zeroed once by the caller and then left alone -- the
    draw counter lives in it and advances on the device, so a captured call draws a new batch on every graph replay."""
    _require_hip(state)
    if state.dtype != torch.int64 or state.numel() != 2 or not state.is_contiguous():
        raise ValueError('state must be a contiguous int64 tensor of 2 elements')
    n = int(n)
    raw = torch.empty((n, 3), dtype=torch.float32, device=state.device)
    norm = torch.empty((n, 3), dtype=torch.float32, device=state.device)
    flat = torch.empty(n, dtype=torch.int64, device=state.device) if want_flat else None
    if n == 0:                          # no draw: the counter in `state` stays where it is, as the entry has it for n = 0
        return (raw, norm, flat) if want_flat else (raw, norm)
    r3 = (ctypes.c_int32 * 3)(*[int(x) for x in res])
    check(_lib.load().lfgc_lattice_sample_f32(int(seed) & 0xFFFFFFFFFFFFFFFF, state.data_ptr(), n, r3, _float3(min_idx), _float3(max_idx),
                                              _float3(scales), raw.data_ptr(), norm.data_ptr(),
                                              flat.data_ptr() if want_flat else None, _stream(state)),
          'lfgc_lattice_sample_f32')
    return (raw, norm, flat) if want_flat else (raw, norm)


# Gradient seed of a scalar loss that GtMseLossFn.backward recognises by identity and does not multiply by: one fill
# and one elementwise launch less per train step than `loss.backward()` (autograd's ones_like + `d_pred * g`).  Read-only.
_UNIT_GRADS = {}


def unit_grad(device) -> torch.Tensor:
    """0-d fp32 tensor holding 1.0 on `device` (cached; create it before capturing a graph): `loss.backward(unit_grad(dev))`."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    t = _UNIT_GRADS.get(device)
    if t is None:
        t = _UNIT_GRADS[device] = torch.ones((), dtype=torch.float32, device=device)
    return t


@_on_device
def deviation_partial(pred: torch.Tensor, gt: torch.Tensor, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """acc = [sum sq, sum abs, min gt, max gt] (fp64, device)."""
    lib = _lib.load()
    _require_hip(pred, gt)
    pred, gt = _f32c(pred).reshape(-1), _f32c(gt).reshape(-1)
    if acc is None:
        acc = torch.tensor([0.0, 0.0, float('inf'), float('-inf')], dtype=torch.float64, device=pred.device)
    if pred.numel() == 0:
        return acc
    check(lib.lfgc_deviation_partial_f32(pred.data_ptr(), gt.data_ptr(), pred.numel(), acc.data_ptr(), _stream(pred)),
          'lfgc_deviation_partial_f32')
    return acc


# ---- direct volume rendering: the ray bookkeeping around the forward kernel -------------------------

def _ray_i32(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError('%s must be a contiguous int32 tensor' % what)
    return t


def _ray_f32x4(t: torch.Tensor, what: str, rows: Optional[int] = None) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != 4 or rows not in (None, t.shape[0]):
        raise ValueError('%s must be a contiguous fp32 (R, 4) tensor' % what)
    return t


def _tf_table(tf_table: torch.Tensor, v_min: float, v_max: float) -> Tuple[int, float]:
    """(K, tf_scale) of a (K, 4) table over [v_min, v_max]: row u = (v - v_min) * tf_scale holds value v."""
    K = int(tf_table.shape[0])
    if tf_table.dim() != 2 or tf_table.shape[1] != 4 or K < 2 or tf_table.dtype != torch.float32 or not tf_table.is_contiguous():
        raise ValueError('tf_table must be a contiguous fp32 (K, 4) tensor with K >= 2')
    if not float(v_max) > float(v_min):
        raise ValueError('v_max must exceed v_min')
    return K, (K - 1) / (float(v_max) - float(v_min))


@_on_device
def ray_clip(origins: torch.Tensor, dirs: torch.Tensor, box_min, box_max, dt: float, max_steps: int,
             t_min: float = 0.0, t_max: float = float('inf')) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(t_near (R,), t_far (R,), n_steps (R,) int32) of R rays against the box: lfgc_ray_clip_f32.  A miss has n_steps 0.
    origins, dirs (R,3); dirs are unit vectors."""
    _require_hip(origins, dirs)
    origins, dirs = _f32c(origins), _f32c(dirs)
    if origins.dim() != 2 or origins.shape[1] != 3 or dirs.shape != origins.shape:
        raise ValueError('origins and dirs must both be (R, 3), got %s and %s' % (tuple(origins.shape), tuple(dirs.shape)))
    R = origins.shape[0]
    t_near = torch.empty(R, dtype=torch.float32, device=origins.device)
    t_far = torch.empty(R, dtype=torch.float32, device=origins.device)
    n_steps = torch.empty(R, dtype=torch.int32, device=origins.device)
    if R:
        check(_lib.load().lfgc_ray_clip_f32(origins.data_ptr(), dirs.data_ptr(), R, _float3(box_min), _float3(box_max), float(t_min),
                                            float(t_max), float(dt), int(max_steps), t_near.data_ptr(), t_far.data_ptr(),
                                            n_steps.data_ptr(), _stream(origins)), 'lfgc_ray_clip_f32')
    return t_near, t_far, n_steps


@_on_device
def ray_samples(live: torch.Tensor, origins: torch.Tensor, dirs: torch.Tensor, t_near: torch.Tensor, t_far: torch.Tensor,
                n_steps: torch.Tensor, k_next: torch.Tensor, dt: float, S: int = 32) -> torch.Tensor:
    """(len(live) * S, 3) positions: row j*S + s is sample k_next[ray] + s of ray live[j] (lfgc_ray_samples_f32).  S is a
    multiple of 32; rows past a ray's last step repeat its last valid sample."""
    _require_hip(live, origins, dirs, t_near, t_far, n_steps, k_next)
    live = _ray_i32(live, 'live')
    pos = torch.empty((live.numel() * int(S), 3), dtype=torch.float32, device=live.device)
    if live.numel():
        check(_lib.load().lfgc_ray_samples_f32(live.data_ptr(), live.numel(), _f32c(origins).data_ptr(), _f32c(dirs).data_ptr(),
                                               _f32c(t_near).data_ptr(), _f32c(t_far).data_ptr(), _ray_i32(n_steps, 'n_steps').data_ptr(),
                                               _ray_i32(k_next, 'k_next').data_ptr(), float(dt), int(S), pos.data_ptr(),
                                               _stream(live)), 'lfgc_ray_samples_f32')
    return pos


@_on_device
def ray_composite(live: torch.Tensor, values: torch.Tensor, grad: Optional[torch.Tensor], dirs: torch.Tensor,
                  t_near: torch.Tensor, t_far: torch.Tensor, n_steps: torch.Tensor, k_next: torch.Tensor, dt: float, S: int,
                  tf_table: torch.Tensor, v_min: float, v_max: float, opacity_limit: float, state: torch.Tensor,
                  ka: float = 0.3, kd: float = 0.7) -> None:
    """Composite the S samples per live ray that ray_samples laid out into state (R,4) in place and advance k_next by S:
    lfgc_ray_composite_f32.  values (len(live)*S,), grad (len(live)*S, 3) or None, tf_table (K,4)."""
    _require_hip(live, values, grad, dirs, t_near, t_far, n_steps, k_next, tf_table, state)
    live = _ray_i32(live, 'live')
    n_rows = live.numel() * int(S)
    K, tf_scale = _tf_table(tf_table, v_min, v_max)
    state = _ray_f32x4(state, 'state')
    values = _f32c(values).reshape(-1)
    if values.numel() != n_rows:
        raise ValueError('%d values for %d rays of %d samples' % (values.numel(), live.numel(), S))
    if grad is not None:
        grad = _f32c(grad)
        if tuple(grad.shape) != (n_rows, 3):
            raise ValueError('grad must be (%d, 3), got %s' % (n_rows, tuple(grad.shape)))
    if not live.numel():
        return
    check(_lib.load().lfgc_ray_composite_f32(live.data_ptr(), live.numel(), values.data_ptr(), _ptr(grad), _f32c(dirs).data_ptr(),
                                             _f32c(t_near).data_ptr(), _f32c(t_far).data_ptr(), _ray_i32(n_steps, 'n_steps').data_ptr(),
                                             _ray_i32(k_next, 'k_next').data_ptr(), float(dt), int(S), tf_table.data_ptr(), K,
                                             float(v_min), tf_scale, float(opacity_limit), float(ka), float(kd), state.data_ptr(),
                                             _stream(live)), 'lfgc_ray_composite_f32')


@_on_device
def ray_composite_preint(live: torch.Tensor, values: torch.Tensor, grad: Optional[torch.Tensor], dirs: torch.Tensor,
                         t_near: torch.Tensor, t_far: torch.Tensor, n_steps: torch.Tensor, k_next: torch.Tensor, dt: float, S: int,
                         tf_table: torch.Tensor, pre: torch.Tensor, v_min: float, v_max: float, opacity_limit: float,
                         state: torch.Tensor, carry_v: torch.Tensor, carry_k: torch.Tensor, ka: float = 0.3,
                         kd: float = 0.7) -> None:
    """``ray_composite`` with pre-integrated classification: every sample composites the slab between itself and the
    sample before it under the table's mean over the slab's value range (lfgc_ray_composite_preint_f32).  pre (K, 4)
    float64 is the integral table of tf_table (Render.TransferFunction.integral_on); carry_v (R,) fp32 and carry_k (R,)
    int32, -1 before a ray's first call, hand a ray's last value from call to call and are updated in place."""
    _require_hip(live, values, grad, dirs, t_near, t_far, n_steps, k_next, tf_table, pre, state, carry_v, carry_k)
    live = _ray_i32(live, 'live')
    n_rows = live.numel() * int(S)
    K, tf_scale = _tf_table(tf_table, v_min, v_max)
    if pre.dtype != torch.float64 or not pre.is_contiguous() or tuple(pre.shape) != (K, 4):
        raise ValueError('pre must be a contiguous float64 (%d, 4) tensor, the integral of tf_table' % K)
    state = _ray_f32x4(state, 'state')
    R = state.shape[0]
    if carry_v.dtype != torch.float32 or not carry_v.is_contiguous() or tuple(carry_v.shape) != (R,):
        raise ValueError('carry_v must be a contiguous fp32 (R,) tensor')
    if tuple(_ray_i32(carry_k, 'carry_k').shape) != (R,):
        raise ValueError('carry_k must be (R,)')
    values = _f32c(values).reshape(-1)
    if values.numel() != n_rows:
        raise ValueError('%d values for %d rays of %d samples' % (values.numel(), live.numel(), S))
    if grad is not None:
        grad = _f32c(grad)
        if tuple(grad.shape) != (n_rows, 3):
            raise ValueError('grad must be (%d, 3), got %s' % (n_rows, tuple(grad.shape)))
    if not live.numel():
        return
    check(_lib.load().lfgc_ray_composite_preint_f32(live.data_ptr(), live.numel(), values.data_ptr(), _ptr(grad),
                                                    _f32c(dirs).data_ptr(), _f32c(t_near).data_ptr(), _f32c(t_far).data_ptr(),
                                                    _ray_i32(n_steps, 'n_steps').data_ptr(), _ray_i32(k_next, 'k_next').data_ptr(),
                                                    float(dt), int(S), tf_table.data_ptr(), K, float(v_min), tf_scale,
                                                    float(opacity_limit), float(ka), float(kd), state.data_ptr(), pre.data_ptr(),
                                                    carry_v.data_ptr(), carry_k.data_ptr(), _stream(live)),
          'lfgc_ray_composite_preint_f32')


def _tf_table2d(tf_table: torch.Tensor, v_min: float, v_max: float, g_max: float) -> Tuple[int, int, float, float]:
    """(Kv, Kg, tf_scale, g_scale) of a (Kv, Kg, 4) table over [v_min, v_max] x [0, g_max]."""
    if (tf_table.dim() != 3 or tf_table.shape[2] != 4 or tf_table.shape[0] < 2 or tf_table.shape[1] < 2
            or tf_table.dtype != torch.float32 or not tf_table.is_contiguous()):
        raise ValueError('tf_table must be a contiguous fp32 (Kv, Kg, 4) tensor with Kv >= 2 and Kg >= 2')
    Kv, Kg = int(tf_table.shape[0]), int(tf_table.shape[1])
    if Kv * Kg > 1 << 22:
        raise ValueError('tf_table has %d x %d entries, more than 2^22' % (Kv, Kg))
    if not float(v_max) > float(v_min):
        raise ValueError('v_max must exceed v_min')
    if not 0.0 < float(g_max) < float('inf'):
        raise ValueError('g_max must be positive and finite')
    return Kv, Kg, (Kv - 1) / (float(v_max) - float(v_min)), (Kg - 1) / float(g_max)


@_on_device
def ray_composite2d(live: torch.Tensor, values: torch.Tensor, grad: torch.Tensor, dirs: torch.Tensor, t_near: torch.Tensor,
                    t_far: torch.Tensor, n_steps: torch.Tensor, k_next: torch.Tensor, dt: float, S: int, tf_table: torch.Tensor,
                    v_min: float, v_max: float, g_max: float, opacity_limit: float, state: torch.Tensor, shade: bool = False,
                    ka: float = 0.3, kd: float = 0.7) -> None:
    """``ray_composite`` under a 2-D table over value and gradient magnitude: lfgc_ray_composite2d_f32.  grad
    (len(live)*S, 3) is required, in the units of ``g_max``; tf_table (Kv, Kg, 4) covers [v_min, v_max] x [0, g_max];
    ``shade`` adds the headlight with ka, kd."""
    _require_hip(live, values, grad, dirs, t_near, t_far, n_steps, k_next, tf_table, state)
    live = _ray_i32(live, 'live')
    n_rows = live.numel() * int(S)
    Kv, Kg, tf_scale, g_scale = _tf_table2d(tf_table, v_min, v_max, g_max)
    state = _ray_f32x4(state, 'state')
    values = _f32c(values).reshape(-1)
    if values.numel() != n_rows:
        raise ValueError('%d values for %d rays of %d samples' % (values.numel(), live.numel(), S))
    if grad is None:
        raise ValueError('a 2-D transfer function needs the gradients: grad is None')
    grad = _f32c(grad)
    if tuple(grad.shape) != (n_rows, 3):
        raise ValueError('grad must be (%d, 3), got %s' % (n_rows, tuple(grad.shape)))
    if not live.numel():
        return
    check(_lib.load().lfgc_ray_composite2d_f32(live.data_ptr(), live.numel(), values.data_ptr(), grad.data_ptr(),
                                               _f32c(dirs).data_ptr(), _f32c(t_near).data_ptr(), _f32c(t_far).data_ptr(),
                                               _ray_i32(n_steps, 'n_steps').data_ptr(), _ray_i32(k_next, 'k_next').data_ptr(),
                                               float(dt), int(S), tf_table.data_ptr(), Kv, Kg, float(v_min), tf_scale, g_scale,
                                               1 if shade else 0, float(opacity_limit), float(ka), float(kd), state.data_ptr(),
                                               _stream(live)), 'lfgc_ray_composite2d_f32')


HISTOGRAM_MAX_BINS = 16384     # Bv * Bg of lfgc_joint_histogram_f32: one 64 KB LDS histogram per workgroup


@_on_device
def joint_histogram(values: torch.Tensor, grad: torch.Tensor, bins, v_min: float, v_max: float, g_max: float,
                    counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """counts (Bv, Bg) int64 += the joint histogram of values (n,) and |grad (n, 3)| over [v_min, v_max] x [0, g_max]:
    lfgc_joint_histogram_f32.  Bin (i, j) is the cell ``ray_composite2d`` interpolates in for a table of (Bv + 1, Bg + 1)
    rows; what lies outside the range falls into the end bins.  ``counts`` None starts from zero; the sums are integers,
    so neither scheduling nor the cut of the samples into calls shows."""
    _require_hip(values, grad, counts)
    Bv, Bg = (int(b) for b in bins)
    if Bv < 1 or Bg < 1 or Bv * Bg > HISTOGRAM_MAX_BINS:
        raise ValueError('bins must be (Bv, Bg) with Bv, Bg >= 1 and Bv * Bg <= %d, got %s' % (HISTOGRAM_MAX_BINS, (Bv, Bg)))
    if not float(v_max) > float(v_min):
        raise ValueError('v_max must exceed v_min')
    if not 0.0 < float(g_max) < float('inf'):
        raise ValueError('g_max must be positive and finite')
    values = _f32c(values).reshape(-1)
    grad = _f32c(grad)
    if tuple(grad.shape) != (values.numel(), 3):
        raise ValueError('grad must be (%d, 3), got %s' % (values.numel(), tuple(grad.shape)))
    if counts is None:
        counts = torch.zeros((Bv, Bg), dtype=torch.int64, device=values.device)
    elif counts.dtype != torch.int64 or not counts.is_contiguous() or tuple(counts.shape) != (Bv, Bg):
        raise ValueError('counts must be a contiguous int64 %s tensor' % ((Bv, Bg),))
    if values.numel():
        check(_lib.load().lfgc_joint_histogram_f32(values.data_ptr(), grad.data_ptr(), values.numel(), Bv, Bg, float(v_min),
                                                   Bv / (float(v_max) - float(v_min)), Bg / float(g_max), counts.data_ptr(),
                                                   _stream(values)), 'lfgc_joint_histogram_f32')
    return counts


@_on_device
def ray_compact(prev: Optional[torch.Tensor], n_steps: torch.Tensor, k_next: torch.Tensor, state: torch.Tensor,
                opacity_limit: float) -> torch.Tensor:
    """The rays of prev (None: all rays) that have steps left (k_next < n_steps) and are not yet opaque
    (1 - T < opacity_limit), in order (int32).  Synchronises once to learn their number."""
    _require_hip(prev, n_steps, k_next, state)
    n_steps, k_next = _ray_i32(n_steps, 'n_steps'), _ray_i32(k_next, 'k_next')
    state = _ray_f32x4(state, 'state', rows=n_steps.numel())
    n = n_steps.numel() if prev is None else _ray_i32(prev, 'prev').numel()
    out = torch.empty(n, dtype=torch.int32, device=n_steps.device)
    if n == 0:
        return out
    count = torch.zeros(1, dtype=torch.int64, device=n_steps.device)
    ws = _select_workspace(n, n_steps.device, 'lfgc_ray_compact_workspace_bytes')
    check(_lib.load().lfgc_ray_compact(_ptr(prev), n, n_steps.data_ptr(), k_next.data_ptr(), state.data_ptr(), float(opacity_limit),
                                       out.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(n_steps)),
          'lfgc_ray_compact')
    return out[:int(count.item())]


# ---- first-hit isosurface ray casting: scan, bisection and hit point around the same forward kernel --

def _iso_value(iso) -> float:
    iso = float(iso)
    if iso != iso or iso in (float('inf'), float('-inf')):
        raise ValueError('iso must be finite')
    return iso


@_on_device
def ray_iso_scan(live: torch.Tensor, values: torch.Tensor, t_near: torch.Tensor, t_far: torch.Tensor, n_steps: torch.Tensor,
                 k_next: torch.Tensor, dt: float, S: int, iso: float, state: torch.Tensor, bracket: torch.Tensor) -> None:
    """Scan the S values per live ray that ray_samples laid out for the first sign change of value - iso:
    lfgc_ray_iso_scan_f32.  A ray with a crossing at sample k gets bracket (t_lo, t_hi, f_lo, f_hi), state.w = 0 and
    k_next = k; the others get their last value into state.x and k_next += S.  state, bracket (R,4), in place."""
    _require_hip(live, values, t_near, t_far, n_steps, k_next, state, bracket)
    live = _ray_i32(live, 'live')
    iso = _iso_value(iso)
    state, bracket = _ray_f32x4(state, 'state'), _ray_f32x4(bracket, 'bracket')
    values = _f32c(values).reshape(-1)
    if values.numel() != live.numel() * int(S):
        raise ValueError('%d values for %d rays of %d samples' % (values.numel(), live.numel(), S))
    if not live.numel():
        return
    check(_lib.load().lfgc_ray_iso_scan_f32(live.data_ptr(), live.numel(), values.data_ptr(), _f32c(t_near).data_ptr(),
                                            _f32c(t_far).data_ptr(), _ray_i32(n_steps, 'n_steps').data_ptr(),
                                            _ray_i32(k_next, 'k_next').data_ptr(), float(dt), int(S), iso, state.data_ptr(),
                                            bracket.data_ptr(), _stream(live)), 'lfgc_ray_iso_scan_f32')


@_on_device
def ray_iso_refine(rays: torch.Tensor, values: Optional[torch.Tensor], origins: torch.Tensor, dirs: torch.Tensor, iso: float,
                   bracket: torch.Tensor) -> torch.Tensor:
    """One bisection step of the brackets of the listed rays (lfgc_ray_iso_refine_f32): values (len(rays),) are the values
    at the midpoints the previous call returned (None: no update), bracket (R,4) is updated in place.  Returns the
    (len(rays), 3) positions of the new midpoints."""
    _require_hip(rays, values, origins, dirs, bracket)
    rays = _ray_i32(rays, 'rays')
    iso = _iso_value(iso)
    bracket = _ray_f32x4(bracket, 'bracket')
    if values is not None:
        values = _f32c(values).reshape(-1)
        if values.numel() != rays.numel():
            raise ValueError('%d values for %d rays' % (values.numel(), rays.numel()))
    pos = torch.empty((rays.numel(), 3), dtype=torch.float32, device=rays.device)
    if rays.numel():
        check(_lib.load().lfgc_ray_iso_refine_f32(rays.data_ptr(), rays.numel(), _ptr(values), _f32c(origins).data_ptr(),
                                                  _f32c(dirs).data_ptr(), iso, bracket.data_ptr(), pos.data_ptr(), _stream(rays)),
              'lfgc_ray_iso_refine_f32')
    return pos


@_on_device
def ray_iso_finish(rays: torch.Tensor, origins: torch.Tensor, dirs: torch.Tensor, bracket: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(t_hit (len(rays),), position (len(rays), 3)) of the listed rays: one secant step inside their final brackets
    (lfgc_ray_iso_finish_f32).  Rows follow the list, not the ray ids."""
    _require_hip(rays, origins, dirs, bracket)
    rays = _ray_i32(rays, 'rays')
    bracket = _ray_f32x4(bracket, 'bracket')
    t_hit = torch.empty(rays.numel(), dtype=torch.float32, device=rays.device)
    pos = torch.empty((rays.numel(), 3), dtype=torch.float32, device=rays.device)
    if rays.numel():
        check(_lib.load().lfgc_ray_iso_finish_f32(rays.data_ptr(), rays.numel(), _f32c(origins).data_ptr(), _f32c(dirs).data_ptr(),
                                                  bracket.data_ptr(), t_hit.data_ptr(), pos.data_ptr(), _stream(rays)),
              'lfgc_ray_iso_finish_f32')
    return t_hit, pos


# ---- empty-space skipping: brick ranges, occupancy under a transfer function, the jump over empty blocks

def _int3(v):
    return (ctypes.c_int32 * 3)(*[int(x) for x in v])


def brick_counts(cells, brick: int) -> Tuple[int, int, int]:
    """Bricks per axis for ``cells`` = res - 1 lattice cells per axis and an edge of ``brick`` cells: ceil(cells / brick)."""
    brick = int(brick)
    if brick < 1 or min(int(c) for c in cells) < 1:
        raise ValueError('brick edge and cells per axis must be >= 1')
    return tuple((int(c) + brick - 1) // brick for c in cells)


def brick_table(res, brick: int, device) -> torch.Tensor:
    """(nbx, nby, nbz, 2) fp32 table of (+inf, -inf) for a lattice of ``res`` points: the start of ops.brick_minmax."""
    t = torch.empty(brick_counts([int(r) - 1 for r in res], brick) + (2,), dtype=torch.float32, device=device)
    t[..., 0], t[..., 1] = float('inf'), float('-inf')
    return t


@_on_device
def brick_minmax(values: torch.Tensor, res, x_begin: int, x_end: int, brick: int, minmax: torch.Tensor) -> torch.Tensor:
    """Fold the lattice planes [x_begin, x_end) of a volume of ``res`` points, given as values (x_end - x_begin, Y, Z), into
    minmax (nbx, nby, nbz, 2) in place (lfgc_brick_minmax_f32); ``brick_table`` makes the empty table."""
    _require_hip(values, minmax)
    res = [int(r) for r in res]
    x_begin, x_end = int(x_begin), int(x_end)
    if values.dtype != torch.float32 or not values.is_contiguous() or tuple(values.shape) != (x_end - x_begin, res[1], res[2]):
        raise ValueError('values must be a contiguous fp32 %s tensor, got %s' % ((x_end - x_begin, res[1], res[2]), tuple(values.shape)))
    want = brick_counts([r - 1 for r in res], brick) + (2,)
    if minmax.dtype != torch.float32 or not minmax.is_contiguous() or tuple(minmax.shape) != want:
        raise ValueError('minmax must be a contiguous fp32 %s tensor' % (want,))
    check(_lib.load().lfgc_brick_minmax_f32(values.data_ptr(), _int3(res), x_begin, x_end, int(brick), minmax.data_ptr(),
                                            _stream(values)), 'lfgc_brick_minmax_f32')
    return minmax


@_on_device
def brick_occupancy(minmax: torch.Tensor, tf_table: torch.Tensor, v_min: float, v_max: float, margin: float) -> torch.Tensor:
    """uint8 table, one entry per brick of minmax (..., 2): 0 where the extinction of tf_table (K, 4) is zero on all of
    [min - margin, max + margin], else 1 (lfgc_brick_occupancy_f32).  v_min, v_max as ops.ray_composite takes them."""
    _require_hip(minmax, tf_table)
    K, tf_scale = _tf_table(tf_table, v_min, v_max)
    if minmax.dtype != torch.float32 or not minmax.is_contiguous() or minmax.dim() < 2 or minmax.shape[-1] != 2:
        raise ValueError('minmax must be a contiguous fp32 (..., 2) tensor')
    if not float(margin) >= 0.0:
        raise ValueError('margin must be >= 0')
    occ = torch.empty(minmax.shape[:-1], dtype=torch.uint8, device=minmax.device)
    if occ.numel():
        check(_lib.load().lfgc_brick_occupancy_f32(minmax.data_ptr(), occ.numel(), tf_table.data_ptr(), K, float(v_min), tf_scale,
                                                   float(margin), occ.data_ptr(), _stream(minmax)), 'lfgc_brick_occupancy_f32')
    return occ


@_on_device
def ray_skip(live: Optional[torch.Tensor], origins: torch.Tensor, dirs: torch.Tensor, t_near: torch.Tensor, t_far: torch.Tensor,
             n_steps: torch.Tensor, k_next: torch.Tensor, dt: float, S: int, box_min, box_max, cells, brick: int,
             occ: torch.Tensor, skipped: torch.Tensor) -> None:
    """Advance k_next of the rays of live (None: all rays) by S while none of their next S samples touches an occupied
    brick, and count the jumps in skipped (R,) int32, both in place: lfgc_ray_skip_f32.  occ (nbx, nby, nbz) uint8 for
    ``cells`` lattice cells per axis and bricks of ``brick`` cells."""
    _require_hip(live, origins, dirs, t_near, t_far, n_steps, k_next, occ, skipped)
    n_steps, k_next, skipped = _ray_i32(n_steps, 'n_steps'), _ray_i32(k_next, 'k_next'), _ray_i32(skipped, 'skipped')
    if skipped.numel() != n_steps.numel() or k_next.numel() != n_steps.numel():
        raise ValueError('n_steps, k_next and skipped must have one entry per ray')
    cells = [int(c) for c in cells]
    if occ.dtype != torch.uint8 or not occ.is_contiguous() or tuple(occ.shape) != brick_counts(cells, brick):
        raise ValueError('occ must be a contiguous uint8 %s tensor, got %s' % (brick_counts(cells, brick), tuple(occ.shape)))
    n = n_steps.numel() if live is None else _ray_i32(live, 'live').numel()
    if not n:
        return
    check(_lib.load().lfgc_ray_skip_f32(_ptr(live), n, _f32c(origins).data_ptr(), _f32c(dirs).data_ptr(), _f32c(t_near).data_ptr(),
                                        _f32c(t_far).data_ptr(), n_steps.data_ptr(), k_next.data_ptr(), float(dt), int(S),
                                        _float3(box_min), _float3(box_max), _int3(cells), int(brick), occ.data_ptr(),
                                        skipped.data_ptr(), _stream(n_steps)), 'lfgc_ray_skip_f32')


# ---- isosurface triangle meshes: classification, compaction and connectivity of one x-slab ------------

def _mesh_slab(values: torch.Tensor, n_owner: int):
    if values.dtype != torch.float32 or not values.is_contiguous() or values.dim() != 3:
        raise ValueError('values must be a contiguous fp32 (nx, Y, Z) tensor')
    nx, ny, nz = (int(v) for v in values.shape)
    n_owner = int(n_owner)
    if not 1 <= n_owner <= nx or ny < 2 or nz < 2:
        raise ValueError('a slab needs 1 <= n_owner <= nx planes and Y, Z >= 2, got n_owner %d of %s' % (n_owner, (nx, ny, nz)))
    return nx, n_owner, ny, nz


@_on_device
def iso_mesh_count(values: torch.Tensor, n_owner: int, iso: float) -> Tuple[torch.Tensor, int, int]:
    """(workspace, vertices, triangles) of the slab ``values`` (nx, Y, Z) whose first n_owner planes own their edges:
    lfgc_iso_mesh_count_f32.  The workspace goes to iso_mesh_emit unchanged.  Synchronises once to read the two totals."""
    _require_hip(values)
    iso = _iso_value(iso)
    nx, n_owner, ny, nz = _mesh_slab(values, n_owner)
    lib = _lib.load()
    nbytes = int(lib.lfgc_iso_mesh_workspace_bytes(nx, n_owner, ny, nz))
    ws = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.int64, device=values.device)
    totals = torch.zeros(2, dtype=torch.int64, device=values.device)
    check(lib.lfgc_iso_mesh_count_f32(values.data_ptr(), nx, n_owner, ny, nz, iso, totals.data_ptr(), ws.data_ptr(),
                                      ws.numel() * 8, _stream(values)), 'lfgc_iso_mesh_count_f32')
    n_vertices, n_triangles = totals.tolist()
    return ws, int(n_vertices), int(n_triangles)


@_on_device
def iso_mesh_emit(values: torch.Tensor, n_owner: int, iso: float, xs: torch.Tensor, ys: torch.Tensor, zs: torch.Tensor,
                  vertex_base: int, workspace: torch.Tensor, n_vertices: int, n_triangles: int):
    """(origins (n,3), dirs (n,3), bracket (n,4), triangles (T,3) int32) of the slab iso_mesh_count has just classified:
    lfgc_iso_mesh_emit_f32.  xs (nx,), ys (Y,), zs (Z,): the coordinates of the slab's planes, rows and columns; triangle
    indices are vertex_base + the slab's ranks.  The brackets are finished by ray_iso_refine / ray_iso_finish."""
    _require_hip(values, xs, ys, zs, workspace)
    iso = _iso_value(iso)
    nx, n_owner, ny, nz = _mesh_slab(values, n_owner)
    xs, ys, zs = _f32c(xs), _f32c(ys), _f32c(zs)
    if (xs.numel(), ys.numel(), zs.numel()) != (nx, ny, nz):
        raise ValueError('axis tables of %d, %d, %d entries for a slab of %s' % (xs.numel(), ys.numel(), zs.numel(), (nx, ny, nz)))
    n_vertices, n_triangles, vertex_base = int(n_vertices), int(n_triangles), int(vertex_base)
    if n_vertices < 0 or n_triangles < 0 or not 0 <= vertex_base < 2 ** 31:
        raise ValueError('n_vertices, n_triangles must be >= 0 and vertex_base in [0, 2^31)')
    if workspace.dtype != torch.int64 or not workspace.is_contiguous():
        raise ValueError('workspace must be the tensor iso_mesh_count returned')
    dev = values.device
    origins = torch.empty((n_vertices, 3), dtype=torch.float32, device=dev)
    dirs = torch.empty((n_vertices, 3), dtype=torch.float32, device=dev)
    bracket = torch.empty((n_vertices, 4), dtype=torch.float32, device=dev)
    triangles = torch.empty((n_triangles, 3), dtype=torch.int32, device=dev)
    check(_lib.load().lfgc_iso_mesh_emit_f32(values.data_ptr(), nx, n_owner, ny, nz, iso, xs.data_ptr(), ys.data_ptr(), zs.data_ptr(),
                                             vertex_base, workspace.data_ptr(), workspace.numel() * 8, n_vertices, n_triangles,
                                             _ptr(origins), _ptr(dirs), _ptr(bracket), _ptr(triangles), _stream(values)),
          'lfgc_iso_mesh_emit_f32')
    return origins, dirs, bracket, triangles


# ---- structural similarity: plane sums of the SSIM of separable, valid-only windows --------------------

SSIM_MAX_WINDOW = 16           # taps per axis of lfgc_ssim_planes_f32


def ssim_window_counts(shape, lengths, strides) -> Tuple[int, int, int]:
    """Windows per axis, (n - w) // s + 1.  ValueError, naming the axis, for a window longer than its extent, a window
    outside 1..16 and a stride below 1."""
    shape, lengths, strides = tuple(int(v) for v in shape), tuple(int(v) for v in lengths), tuple(int(v) for v in strides)
    if len(shape) != 3 or len(lengths) != 3 or len(strides) != 3:
        raise ValueError('SSIM takes 3-D arrays with one window and one stride per axis, got shape %s, windows %s, strides %s'
                         % (shape, lengths, strides))
    for axis, (n, w, s) in enumerate(zip(shape, lengths, strides)):
        if not 1 <= w <= SSIM_MAX_WINDOW:
            raise ValueError('the window of axis %d has %d taps: 1..%d are supported' % (axis, w, SSIM_MAX_WINDOW))
        if s < 1:
            raise ValueError('the stride of axis %d is %d: it must be at least 1' % (axis, s))
        if w > n:
            raise ValueError('the window of axis %d (%d taps) is longer than the extent %d' % (axis, w, n))
    return tuple((n - w) // s + 1 for n, w, s in zip(shape, lengths, strides))


@_on_device
def ssim_plane_sums(a: torch.Tensor, b: torch.Tensor, windows, strides, c1: float, c2: float, cov_norm: float = 1.0,
                    want_map: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(plane_sums (m0,) fp64, map (m0, m1, m2) fp64 or None) on the device: lfgc_ssim_planes_f32 of two (n0, n1, n2)
    tensors.  ``windows`` holds the three axes' weights (each normalised to sum 1, 1..16 taps), ``strides`` three ints;
    c1, c2 and cov_norm are those of the formula.  plane_sums[i0] adds the SSIM of the windows (i0, ., .) in an order
    that does not depend on n0, so the planes of a sub-array a[x0:x1] come out with the bits they have in the whole."""
    if a.shape != b.shape:
        raise ValueError('the two arrays differ in shape: %s and %s' % (tuple(a.shape), tuple(b.shape)))
    weights = [np.ascontiguousarray(np.asarray(g, dtype=np.float64).reshape(-1)) for g in windows]
    if len(weights) != 3:
        raise ValueError('windows must hold the weights of the three axes, got %d entries' % len(weights))
    lengths = [int(g.size) for g in weights]
    m = ssim_window_counts(a.shape, lengths, strides)
    if not all(np.isfinite(g).all() for g in weights):
        raise ValueError('window weights must be finite')
    c1, c2, cov_norm = float(c1), float(c2), float(cov_norm)
    if not (0.0 < c1 < float('inf') and 0.0 < c2 < float('inf') and 0.0 < cov_norm < float('inf')):
        raise ValueError('c1, c2 and cov_norm must be positive and finite, got %r, %r, %r' % (c1, c2, cov_norm))
    _require_hip(a, b)
    a, b = _f32c(a.detach()), _f32c(b.detach())
    n = [int(v) for v in a.shape]
    lib = _lib.load()
    w_arr = (ctypes.c_int * 3)(*lengths)
    s_arr = (ctypes.c_int * 3)(*[int(v) for v in strides])
    flat = np.concatenate(weights)
    nbytes = int(lib.lfgc_ssim_workspace_bytes(n[0], n[1], n[2], w_arr, s_arr))
    if nbytes <= 0:
        raise _lib.LfgcError('lfgc_ssim_planes_f32 refuses an array of %s with windows %s and strides %s: too many windows '
                             'for one call' % (tuple(n), tuple(lengths), tuple(int(v) for v in strides)))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
    sums = torch.empty(m[0], dtype=torch.float64, device=a.device)
    smap = torch.empty(m, dtype=torch.float64, device=a.device) if want_map else None
    check(lib.lfgc_ssim_planes_f32(a.data_ptr(), b.data_ptr(), n[0], n[1], n[2], flat.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                   w_arr, s_arr, c1, c2, cov_norm, sums.data_ptr(), _ptr(smap), ws.data_ptr(), nbytes, _stream(a)),
          'lfgc_ssim_planes_f32')
    return sums, smap
