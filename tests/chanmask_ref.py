"""REFERENCE (test infrastructure, NOT product code) -- numpy restatement of mode 2 of the checkpoint codec's mask file, the
pruning mask once per cell, written from the format in DESIGN.md section 3.6 and not from the kernels.

A tensor t of numel_t coefficients is x_t[c, j], c < C channels, j < S_t = numel_t / C cells, in its flat order.

    u8  2
    u32 K[n_grids]     K[t] = cells of tensor t with a non-zero coefficient in any channel
    field support      sum_t S_t bits: bit sum_{u<t} S_u + j = any_c x_t[c, j] != 0
    field residual     C * sum_t K[t] bits: bit C * sum_{u<t} K[u] + c * K[t] + r = x_t[c, j_r] != 0, j_r the r-th support cell
    field = u8 m, then m = 0: ceil(bits / 8) plain bytes, MSB first, tail bits zero;  m = 1: one rANS stream over those bytes

A field takes m = 1 only where that is strictly smaller.  The rANS coder is tests/rans_ref.py.
"""
from __future__ import annotations

import struct
from typing import List, Sequence, Tuple

import numpy as np

import rans_ref as A


def factor(mask, C: int) -> Tuple[np.ndarray, np.ndarray]:
    """(support (S,) bool, residual (C * K,) bool) of one tensor's flat mask (numel,) bool."""
    m = np.asarray(mask, dtype=bool).reshape(C, -1)
    support = m.any(axis=0)
    return support, m[:, support].reshape(-1)


def unfactor(support, residual, C: int) -> np.ndarray:
    """The flat mask (C * S,) bool back from its support and residual."""
    support = np.asarray(support, dtype=bool)
    K = int(support.sum())
    residual = np.asarray(residual, dtype=bool)
    assert residual.size == C * K
    m = np.zeros((C, support.size), dtype=bool)
    m[:, support] = residual.reshape(C, K)
    return m.reshape(-1)


def field(bits, R: int = A.ROUNDS) -> bytes:
    plain = np.packbits(np.asarray(bits, dtype=np.uint8)).tobytes()
    if not plain:
        return b'\x00'
    return A.coded(plain, A.encode(np.frombuffer(plain, np.uint8), R))


def write_mask_file(masks: Sequence[np.ndarray], C: int, R: int = A.ROUNDS) -> bytes:
    """The mode-2 mask file of the tensors' flat masks."""
    parts = [factor(m, C) for m in masks]
    out = bytes([2]) + b''.join(struct.pack('<I', int(s.sum())) for s, _ in parts)
    out += field(np.concatenate([s for s, _ in parts]), R)
    out += field(np.concatenate([r for _, r in parts]), R)
    return out


def flat_mask_file(masks: Sequence[np.ndarray], R: int = A.ROUNDS) -> bytes:
    """What entropy=True alone writes: mode 0 or 1 over the flat mask of all tensors."""
    plain = np.packbits(np.concatenate([np.asarray(m, dtype=np.uint8).reshape(-1) for m in masks])).tobytes()
    return A.coded(plain, A.encode(np.frombuffer(plain, np.uint8), R))


def best_mask_file(masks: Sequence[np.ndarray], C: int, R: int = A.ROUNDS) -> bytes:
    """What channel_mask=True writes: the strictly smallest of modes 0, 1 and 2, ties to the lower mode."""
    flat, per_cell = flat_mask_file(masks, R), write_mask_file(masks, C, R)
    return per_cell if len(per_cell) < len(flat) else flat


def _take_field(buf: bytes, at: int, nbits: int) -> Tuple[np.ndarray, int, int]:
    nbytes = (nbits + 7) // 8
    m = buf[at]
    at += 1
    if m == 0:
        data = np.frombuffer(buf[at:at + nbytes], np.uint8)
        assert data.size == nbytes, 'truncated field'
        at += nbytes
    else:
        assert m == 1, 'field mode %d' % m
        info = A.stream_info(buf, at)
        data = A.decode(buf[at:at + info['nbytes']])
        assert data.size == nbytes
        at += info['nbytes']
    return np.unpackbits(data)[:nbits].astype(bool), at, m


def parse_mask_file(buf: bytes, numels: Sequence[int], C: int) -> Tuple[List[np.ndarray], List[int], List[int]]:
    """([flat mask of every tensor], K, [field modes]) of a mode-2 mask file for tensors of `numels` coefficients."""
    assert buf[0] == 2
    n = len(numels)
    K = list(struct.unpack_from('<%dI' % n, buf, 1))
    S = [v // C for v in numels]
    assert all(v % C == 0 for v in numels) and all(k <= s for k, s in zip(K, S))
    support, at, m0 = _take_field(buf, 1 + 4 * n, sum(S))
    residual, at, m1 = _take_field(buf, at, C * sum(K))
    assert at == len(buf), 'trailing bytes'
    masks, s_at, r_at = [], 0, 0
    for s, k in zip(S, K):
        sup = support[s_at:s_at + s]
        assert int(sup.sum()) == k
        masks.append(unfactor(sup, residual[r_at:r_at + C * k], C))
        s_at += s
        r_at += C * k
    return masks, K, [m0, m1]
