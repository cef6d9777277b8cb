"""Error-bounded volumes: a residual stream beside the compressed model that guarantees a pointwise bound (DESIGN.md 3.6;
the reference has none).  ``store_residuals`` predicts the volume with the model slab by slab, quantises what is left against
the ground truth in steps of twice the bound, entropy-codes the symbols and stores verbatim the voxels that do not fit;
``restore_volume`` repeats the same launches and applies the stream, so that every voxel of its result satisfies
``abs(float64(out) - float64(gt)) <= float64(float32(max_error))`` (bit equality where gt is not finite).

File, little-endian::

    b'LFGR' | u8 version = 1 | 3 x u8 0 | u32 X, Y, Z | f32 eps | u32 tiled_res | u32 slab_planes          (32 bytes)
    per x-slab of slab_planes planes (the last one shorter), in x order:
        u32 K | u64 checksum | u8 mode | payload | K x f32 outliers

``u8 mode | payload`` is the codec's field (codec_container.py) -- mode 0: the slab's symbol bytes; mode 1: their rANS
stream (``ops.RANS_ROUNDS`` rounds per chunk), only where it is strictly shorter.  The arithmetic of symbols, outliers and
checksum is the contract of include/lfgc.h; all per-voxel work is HIP (csrc/lfgc_residual.hip, csrc/lfgc_rans.hip), this
module is the slab loop and the bytes."""
from __future__ import annotations

import struct
import warnings
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .. import ops
from ..visualization.OutputToVTK import field_from_net_fused
from .codec_container import Reader, read_field, write_field

MAGIC = b'LFGR'
VERSION = 1
_HEADER = '<4s4B3IfII'
_RECORD = '<IQ'                                  # K, checksum: what stands before a record's field
_SLAB_VOXELS = 1 << 24                           # default slab: at most this many voxels (64 MiB of prediction)


class PredictionMismatch(ValueError):
    """The decoder's prediction of a slab does not have the bits the encoder quantised against: another model, another
    kernel build or another precision.  The error bound does not hold for a volume restored this way."""


def _positive_int(v, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v < 1 << 32:
        raise ValueError('%s must be an integer from 1 to 2^32 - 1, got %r' % (what, v))
    return int(v)


def _slabs(X: int, slab_planes: int):
    """(x0, x1) of every slab in x order; lazily: a header may name billions, and the parser stops at the first one missing."""
    for x0 in range(0, X, slab_planes):
        yield x0, min(x0 + slab_planes, X)


def _default_slab_planes(res, tiled_res: int) -> int:
    """Whole tiles of planes up to _SLAB_VOXELS voxels, at least one plane."""
    planes = max(1, _SLAB_VOXELS // (res[1] * res[2]))
    if planes >= tiled_res:
        planes -= planes % tiled_res
    return min(planes, res[0])


def parse_residual_file(raw: bytes) -> SimpleNamespace:
    """Header and record descriptions of a residual file, on the host (nothing touches the GPU): ``X, Y, Z, eps, tiled_res,
    slab_planes`` and ``records``, one per slab with ``x0, x1, n`` (voxels), ``K, checksum, mode, payload`` (offset, bytes),
    ``rans`` (the stream's header by ``ops.codec_rans_header``, None in mode 0) and ``outliers`` (offset).  ValueError for a
    bad magic or version, a zero dimension, an eps that is no positive normal number, tiled_res or slab_planes < 1, a
    truncated record, an unknown mode, K above the slab's voxel count, a stream of another symbol count than the slab, and
    trailing bytes."""
    r = Reader(raw, 'residual file')
    magic, version, z0, z1, z2, X, Y, Z, eps, tiled_res, slab_planes = r.take(_HEADER)
    if magic != MAGIC or version != VERSION or z0 or z1 or z2:
        raise ValueError('not a residual file of version %d (magic %r, version %d, reserved %d %d %d)'
                         % (VERSION, bytes(magic), version, z0, z1, z2))
    if min(X, Y, Z) < 1:
        raise ValueError('residual file: a volume of %d x %d x %d voxels' % (X, Y, Z))
    try:
        eps = ops.residual_eps(eps)
    except ValueError:
        raise ValueError('residual file: the bound %r is no positive normal fp32 number' % (eps,)) from None
    if tiled_res < 1 or slab_planes < 1:
        raise ValueError('residual file: tiled_res %d, slab_planes %d' % (tiled_res, slab_planes))
    records = []
    for x0, x1 in _slabs(X, slab_planes):
        n = (x1 - x0) * Y * Z
        K, checksum = r.take(_RECORD)
        if K > n:
            raise ValueError('residual file: %d outliers in a slab of %d voxels' % (K, n))
        mode, payload = read_field(r, n, [(n, 256)], length=r.room() - 1 - 4 * K)     # a stream leaves room for the outliers
        data, info = (payload, None) if mode == 0 else payload[0]
        records.append(SimpleNamespace(x0=x0, x1=x1, n=n, K=K, checksum=checksum, mode=mode, payload=(r.at - len(data), len(data)),
                                       rans=info, outliers=r.at))
        r.array('<f4', K)
    r.end()
    return SimpleNamespace(X=X, Y=Y, Z=Z, eps=eps, tiled_res=tiled_res, slab_planes=slab_planes, records=records)


def _device_of(model) -> torch.device:
    if not torch.cuda.is_available():
        raise ops._lib.LfgcError('the residual layer runs its per-voxel work on the MI355X: no GPU is visible. '
                                 'There is no CPU fallback.')
    return next(model.parameters()).device


def store_residuals(dataset, model, gt_vol: torch.Tensor, filename, max_error, tiled_res: int = 32,
                    slab_planes: Optional[int] = None) -> dict:
    """Write ``filename``: what ``restore_volume`` needs beside ``model`` to give back ``gt_vol`` (X, Y, Z fp32, host or
    device) within ``max_error`` at every voxel.  Per x-slab of ``slab_planes`` planes (default: whole tiles up to 2^24
    voxels) one ``field_from_net_fused`` launch, the quantisation, the compaction of the outliers and the rANS coder; device
    memory stays bounded by the slab.  An absolute bound: for one relative to the value range, multiply by the range.
    Returns ``{'bytes', 'escapes', 'voxels', 'bits_per_voxel'}``."""
    eps = ops.residual_eps(max_error)
    tiled_res = _positive_int(tiled_res, 'tiled_res')
    res = tuple(int(v) for v in dataset.vol_res_touple)
    slab_planes = _default_slab_planes(res, tiled_res) if slab_planes is None else _positive_int(slab_planes, 'slab_planes')
    if not torch.is_tensor(gt_vol) or gt_vol.dtype != torch.float32 or tuple(gt_vol.shape) != res:
        raise ValueError('gt_vol must be a float32 tensor of the dataset\'s shape %r' % (res,))
    if slab_planes * res[1] * res[2] >= 1 << 32:
        raise ValueError('a slab of %d planes has 2^32 voxels or more: the entropy coder takes fewer' % slab_planes)
    device = _device_of(model)
    gt_vol = gt_vol.detach().contiguous()
    out = [struct.pack(_HEADER, MAGIC, VERSION, 0, 0, 0, res[0], res[1], res[2], eps, tiled_res, slab_planes)]
    escapes = 0
    for x0, x1 in _slabs(res[0], slab_planes):
        gt = gt_vol[x0:x1].to(device)
        pred = field_from_net_fused(dataset, model, x0, x1, tiled_res)
        sym, checksum = ops.residual_quantize(pred, gt, eps)
        outliers = ops.residual_outliers(sym, gt)
        out.append(struct.pack(_RECORD, outliers.numel(), int(checksum.item()) & 0xFFFFFFFFFFFFFFFF))
        out.append(write_field(sym.cpu().numpy().tobytes(), [ops.codec_rans_encode(sym, ops.RANS_ROUNDS)]))
        out.append(outliers.cpu().numpy().astype('<f4', copy=False).tobytes())
        escapes += outliers.numel()
    blob = b''.join(out)
    with open(filename, 'wb') as f:
        f.write(blob)
    voxels = res[0] * res[1] * res[2]
    return {'bytes': len(blob), 'escapes': escapes, 'voxels': voxels, 'bits_per_voxel': 8.0 * len(blob) / voxels}


def restore_volume(dataset, model, filename, strict: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (X, Y, Z) device volume of ``filename`` over ``model``: the launches of ``store_residuals`` again, with the
    ``tiled_res`` and ``slab_planes`` the file records, then the residual stream applied in place.  Where a slab's prediction
    does not have the checksum the encoder stored, ``PredictionMismatch`` (a ValueError); with ``strict=False`` a warning
    instead -- the volume is returned and the bound is void.  ValueError after the slab where the symbols hold another number
    of escapes than the record's K."""
    with open(filename, 'rb') as f:
        raw = f.read()
    info = parse_residual_file(raw)
    res = tuple(int(v) for v in dataset.vol_res_touple)
    if res != (info.X, info.Y, info.Z):
        raise ValueError('the file holds a volume of %d x %d x %d voxels, the dataset one of %r' % (info.X, info.Y, info.Z, res))
    device = _device_of(model)
    if out is None:
        out = torch.empty(res, dtype=torch.float32, device=device)
    elif (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != res or not out.is_contiguous()
          or out.device != device):
        raise ValueError('out must be a contiguous float32 tensor of shape %r on %s' % (res, device))
    host = np.frombuffer(raw, np.uint8)
    for rec in info.records:
        at, nbytes = rec.payload
        payload = torch.from_numpy(host[at:at + nbytes].copy()).to(device)
        with torch.cuda.device(device):
            sym = payload if rec.mode == 0 else ops.codec_rans_decode_parsed(payload, rec.rans)
        outliers = torch.from_numpy(host[rec.outliers:rec.outliers + 4 * rec.K].copy().view('<f4')).to(device)
        slab = out[rec.x0:rec.x1]
        pred = field_from_net_fused(dataset, model, rec.x0, rec.x1, info.tiled_res, out=slab)
        _, checksum, n_escape, status = ops.residual_apply(pred, sym, info.eps, outliers, out=pred)
        found, code = int(n_escape.item()), int(status.item())
        if found != rec.K or code:
            raise ValueError('residual file: the symbols of planes %d to %d hold %d escapes, the record %d outliers (status %d)'
                             % (rec.x0, rec.x1, found, rec.K, code))
        if int(checksum.item()) & 0xFFFFFFFFFFFFFFFF != rec.checksum:
            what = ('planes %d to %d: the prediction is not the one the residuals were taken against (checksum %016x, stored '
                    '%016x)' % (rec.x0, rec.x1, int(checksum.item()) & 0xFFFFFFFFFFFFFFFF, rec.checksum))
            if strict:
                raise PredictionMismatch(what)
            warnings.warn(what + '; the error bound does not hold for this volume')
    return out
