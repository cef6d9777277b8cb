"""REFERENCE (test infrastructure, NOT product code) -- numpy restatement of the error-bounded residual layer, written from
the contract in DESIGN.md section 3.6 / include/lfgc.h and not from the kernels: the per-voxel arithmetic in np.float32 /
np.float64, the prediction checksum in wrapping uint64, and a writer / reader of the residual file that uses tests/rans_ref.py
for mode 1.  Also the adversarial input mixture the host and GPU tests share."""
from __future__ import annotations

import struct
from typing import List, Tuple

import numpy as np

import rans_ref as A

ESCAPE = 255
HEADER = struct.Struct('<4s4B3IfII')
RECORD = struct.Struct('<IQB')


def steps(max_error) -> Tuple[np.float32, np.float32, np.float32]:
    eps = np.float32(max_error)
    step = np.float32(eps + eps)
    return eps, step, np.float32(np.float32(1.0) / step)


def quantise(p, g, max_error, detail: bool = False):
    """Symbols (uint8) of prediction p against truth g; with `detail` also the masks of the first and the second escape
    test (range / non-finite, and the bound itself in double)."""
    p, g = np.asarray(p, np.float32).reshape(-1), np.asarray(g, np.float32).reshape(-1)
    eps, step, inv = steps(max_error)
    with np.errstate(all='ignore'):
        t = ((g - p).astype(np.float32) * inv).astype(np.float32)
        q = np.rint(t)                                                         # ties to even
        first = ~(np.abs(q) <= np.float32(127.0))
        qi = np.where(first, 0, q).astype(np.int32)
        r = (p + (qi.astype(np.float32) * step).astype(np.float32)).astype(np.float32)
        second = ~first & ~(np.abs(g.astype(np.float64) - r.astype(np.float64)) <= np.float64(eps))
    sym = ((qi << 1) ^ (qi >> 31)).astype(np.int64) & 0xFF
    sym = np.where(first | second, ESCAPE, sym).astype(np.uint8)
    return (sym, first, second) if detail else sym


def checksum(p) -> int:
    bits = np.asarray(p, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    w = np.arange(bits.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    with np.errstate(over='ignore'):
        return int(np.sum(bits * w, dtype=np.uint64))


def outliers(sym, g) -> np.ndarray:
    return np.asarray(g, np.float32).reshape(-1)[np.asarray(sym).reshape(-1) == ESCAPE].copy()


def apply(p, sym, max_error, out_values) -> np.ndarray:
    """What the symbols decode to over prediction p, the escapes taking out_values in order (all of them must be there)."""
    p, sym = np.asarray(p, np.float32).reshape(-1), np.asarray(sym, np.uint8).reshape(-1)
    _, step, _ = steps(max_error)
    s = sym.astype(np.int32)
    qi = (s >> 1) ^ -(s & 1)
    with np.errstate(all='ignore'):
        r = (p + (qi.astype(np.float32) * step).astype(np.float32)).astype(np.float32)
    esc = sym == ESCAPE
    assert int(esc.sum()) == np.asarray(out_values).size
    out = r.view(np.uint32).copy()
    out[esc] = np.asarray(out_values, np.float32).view(np.uint32)
    return out.view(np.float32)


def violations(out, gt, max_error) -> np.ndarray:
    """Indices where the guarantee fails: |float64(out) - float64(gt)| <= float64(float32(eps)), bit equality where gt is
    not finite.  Uses nothing of the functions above."""
    out, gt = np.asarray(out, np.float32).reshape(-1), np.asarray(gt, np.float32).reshape(-1)
    fin = np.isfinite(gt)
    with np.errstate(all='ignore'):
        ok = np.where(fin, np.abs(out.astype(np.float64) - gt.astype(np.float64)) <= np.float64(np.float32(max_error)),
                      out.view(np.uint32) == gt.view(np.uint32))
    return np.flatnonzero(~ok)


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def adversarial(max_error) -> Tuple[np.ndarray, np.ndarray]:
    """(p, g): half-step ties, g == p, signed zeros, residuals of 126.5, 127.5 and 1e6 steps, NaN and +-Inf on either side."""
    _, step, _ = steps(max_error)
    st = np.float64(step)
    p, g = [], []
    for k in (-3, -2, -1, 0, 1, 2):                                            # t = k + 0.5 where the products are exact
        p.append(0.0), g.append((k + 0.5) * st)
    for k in (-2.5, 0.5, 1.5):
        p.append(0.75), g.append(np.float64(np.float32(0.75)) + k * st)
    for v in (0.25, -0.6, 1.0):
        p.append(v), g.append(v)
    for a, b in ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0)):
        p.append(a), g.append(b)
    for c in (126.5, 127.5, 1e6):
        for sgn in (1.0, -1.0):
            p.append(0.125), g.append(0.125 + sgn * c * st)
    nan, inf = float('nan'), float('inf')
    for v in (nan, inf, -inf):
        p.append(0.3), g.append(v)
        p.append(v), g.append(0.3)
    p.append(inf), g.append(inf)
    p.append(nan), g.append(nan)
    p, g = np.array(p, np.float32), np.array(g, np.float32)
    g.view(np.uint32)[-1] = 0x7FC12345                                         # a NaN payload that must come back bit for bit
    return p, g


def mixture(n: int, max_error, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """n voxels: values near 1 whose residual spreads over +-40 steps (at eps = 1e-6 the rounding of r, half an ulp of 1 =
    6e-8, is 6 % of the bound, so the second escape test fires), with the adversarial pairs laid over them: all of them
    from a rotating start for a small n, sprinkled over a quarter of the positions for a large one."""
    rng = np.random.default_rng(seed)
    _, step, _ = steps(max_error)
    p = rng.uniform(0.5, 1.5, n).astype(np.float32)
    g = (p.astype(np.float64) + rng.uniform(-40.0, 40.0, n) * np.float64(step)).astype(np.float32)
    ap, ag = adversarial(max_error)
    if n <= 4 * ap.size:
        take = (np.arange(min(n, ap.size)) + seed) % ap.size
        at = rng.permutation(n)[:take.size]
    else:
        at = rng.permutation(n)[:n // 4]
        take = rng.integers(0, ap.size, at.size)
    p[at], g[at] = ap[take], ag[take]
    return p, g


# ---- the file ----------------------------------------------------------------------------------------------------------------

def slabs(X: int, slab_planes: int) -> List[Tuple[int, int]]:
    return [(x0, min(x0 + slab_planes, X)) for x0 in range(0, X, slab_planes)]


def write_file(pred, gt, max_error, tiled_res: int, slab_planes: int, force_mode=None) -> Tuple[bytes, List[int]]:
    """(file, mode per record) for the prediction volume `pred` (X, Y, Z) the encoder saw; `force_mode` 0 writes every record
    plain (the size the coded file must beat)."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    X, Y, Z = pred.shape
    eps, _, _ = steps(max_error)
    out = [HEADER.pack(b'LFGR', 1, 0, 0, 0, X, Y, Z, eps, tiled_res, slab_planes)]
    modes = []
    for x0, x1 in slabs(X, slab_planes):
        p, g = pred[x0:x1].reshape(-1), gt[x0:x1].reshape(-1)
        sym = quantise(p, g, eps)
        esc = outliers(sym, g)
        plain = sym.tobytes()
        field = b'\x00' + plain if force_mode == 0 else A.coded(plain, A.encode(sym, A.ROUNDS))
        modes.append(field[0])
        out.append(struct.pack('<IQ', esc.size, checksum(p)) + field + esc.astype('<f4').tobytes())
    return b''.join(out), modes


def read_file(raw: bytes) -> dict:
    """Header fields and, per record, x0, x1, K, checksum, mode, the decoded symbols and the outliers."""
    magic, version, z0, z1, z2, X, Y, Z, eps, tiled_res, slab_planes = HEADER.unpack_from(raw, 0)
    assert magic == b'LFGR' and version == 1 and (z0, z1, z2) == (0, 0, 0)
    at, records = HEADER.size, []
    for x0, x1 in slabs(X, slab_planes):
        n = (x1 - x0) * Y * Z
        K, cks, mode = RECORD.unpack_from(raw, at)
        at += RECORD.size
        if mode == 0:
            sym = np.frombuffer(raw, np.uint8, n, at)
            at += n
        else:
            info = A.stream_info(raw, at)
            sym = A.decode(raw[at:at + info['nbytes']])
            assert sym.size == n
            at += info['nbytes']
        esc = np.frombuffer(raw, '<f4', K, at)
        at += 4 * K
        records.append(dict(x0=x0, x1=x1, K=K, checksum=cks, mode=mode, sym=sym, outliers=esc))
    assert at == len(raw)
    return dict(X=X, Y=Y, Z=Z, eps=np.float32(eps), tiled_res=tiled_res, slab_planes=slab_planes, records=records)


def restore(raw: bytes, pred) -> np.ndarray:
    """The volume of a file over the decoder's prediction; ValueError where a slab's checksum differs."""
    f = read_file(raw)
    pred = np.asarray(pred, np.float32)
    out = np.empty((f['X'], f['Y'], f['Z']), np.float32)
    for r in f['records']:
        p = pred[r['x0']:r['x1']].reshape(-1)
        if checksum(p) != r['checksum']:
            raise ValueError('prediction mismatch')
        out[r['x0']:r['x1']] = apply(p, r['sym'], f['eps'], r['outliers']).reshape(out[r['x0']:r['x1']].shape)
    return out
