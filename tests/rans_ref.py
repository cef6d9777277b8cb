"""REFERENCE (test infrastructure, NOT product code) -- numpy restatement of the checkpoint codec's entropy stage, written
from the format in DESIGN.md section 3.6 and not from the kernels: the frequency normalisation, the 64-lane interleaved
rANS coder and decoder, and a writer / parser for entropy-mode parameter and mask files.

Stream (little-endian):  u32 n | u16 R | u16 0 | u16 f[256] | u32 words[nc]  then per chunk  u32 state[64], u16 word[words[c]]
with nc = ceil(n / 64R).  Byte-symbol rANS, static order-0 model, frequencies summing to 4096, 32-bit state in
[2^16, 2^32), 16-bit renormalisation, initial encoder state 2^16; lane l of a chunk codes chunk positions 64 r + l.
"""
from __future__ import annotations

import struct
from typing import Dict, List, Tuple

import numpy as np

from oracle import ref_codec as K

M_BITS = 12
M = 1 << M_BITS
LOW = 1 << 16
HEADER = 8 + 2 * 256
ROUNDS = 512                                        # what the file writer uses


def normalise(h) -> np.ndarray:
    """256 counts -> 256 frequencies summing to 4096 (int64)."""
    h = [int(v) for v in np.asarray(h).reshape(-1)]
    assert len(h) == 256 and min(h) >= 0
    n = sum(h)
    assert n > 0
    f = [0 if v == 0 else max(1, v * M // n) for v in h]
    d = M - sum(f)
    order = sorted(range(256), key=lambda s: (-h[s], s))
    while d != 0:
        for s in order:
            if d > 0 and h[s] > 0:
                f[s] += 1
                d -= 1
            elif d < 0 and f[s] > 1:
                f[s] -= 1
                d += 1
            if d == 0:
                break
    return np.asarray(f, dtype=np.int64)


def _cum(f: np.ndarray) -> np.ndarray:
    return np.concatenate([[0], np.cumsum(f)])[:256].astype(np.int64)


def chunks_of(n: int, R: int) -> int:
    return -(-n // (64 * R))


def encode_parts(sym, R: int = ROUNDS):
    """(f, states (nc, 64), [words of chunk c]) of the symbols coded with R rounds per chunk."""
    sym = np.asarray(sym, dtype=np.uint8).reshape(-1)
    n = sym.size
    assert n >= 1 and 1 <= R <= 0xFFFF
    f = normalise(np.bincount(sym, minlength=256))
    cum = _cum(f)
    nc = chunks_of(n, R)
    padded = np.zeros(nc * 64 * R, np.uint8)
    padded[:n] = sym
    S = padded.reshape(nc, R, 64)
    act = (np.arange(nc * 64 * R) < n).reshape(nc, R, 64)
    x = np.full((nc, 64), LOW, np.int64)
    E = np.zeros((nc, R, 64), bool)
    V = np.zeros((nc, R, 64), np.uint16)
    for r in range(R - 1, -1, -1):
        s, a = S[:, r], act[:, r]
        fs = np.where(a, f[s], 1)
        e = a & ((x >> 20) >= fs)
        E[:, r] = e
        V[:, r] = (x & 0xFFFF).astype(np.uint16)
        x = np.where(e, x >> 16, x)
        x = np.where(a, ((x // fs) << M_BITS) + x % fs + cum[s], x)
    return f, x, [V[c][E[c]] for c in range(nc)]          # boolean selection: round-major, lane-minor


def assemble(n: int, R: int, f, states, words) -> bytes:
    out = bytearray(struct.pack('<IHH', n, R, 0))
    out += np.asarray(f).astype('<u2').tobytes()
    out += np.asarray([len(w) for w in words]).astype('<u4').tobytes()
    for st, w in zip(states, words):
        out += np.asarray(st).astype('<u4').tobytes()
        out += np.asarray(w).astype('<u2').tobytes()
    return bytes(out)


def encode(sym, R: int = ROUNDS) -> bytes:
    sym = np.asarray(sym, dtype=np.uint8).reshape(-1)
    f, states, words = encode_parts(sym, R)
    return assemble(sym.size, R, f, states, words)


def stream_info(buf: bytes, offset: int = 0, exact: bool = False) -> Dict[str, object]:
    """Header of the stream at buf[offset:]: n, R, f, words, nbytes.  ValueError for a header that cannot be one."""
    if len(buf) - offset < HEADER:
        raise ValueError('truncated rANS stream')
    n, R, zero = struct.unpack_from('<IHH', buf, offset)
    f = np.frombuffer(buf, '<u2', 256, offset + 8).astype(np.int64)
    if R < 1 or zero != 0 or int(f.sum()) != M:
        raise ValueError('not a rANS stream header')
    nc = chunks_of(n, R)
    if len(buf) - offset < HEADER + 4 * nc:
        raise ValueError('truncated rANS stream')
    words = np.frombuffer(buf, '<u4', nc, offset + HEADER).astype(np.int64)
    nbytes = HEADER + 260 * nc + 2 * int(words.sum())
    if len(buf) - offset < nbytes or (exact and len(buf) - offset != nbytes):
        raise ValueError('rANS stream length does not match its word counts')
    return dict(n=n, R=R, f=f, words=words, nbytes=nbytes)


def split(buf: bytes) -> Tuple[Dict[str, object], np.ndarray, List[np.ndarray]]:
    info = stream_info(buf, 0, exact=True)
    nc = info['words'].size
    states, words, at = np.zeros((nc, 64), np.int64), [], HEADER + 4 * nc
    for c in range(nc):
        states[c] = np.frombuffer(buf, '<u4', 64, at)
        at += 256
        words.append(np.frombuffer(buf, '<u2', int(info['words'][c]), at).astype(np.int64))
        at += 2 * int(info['words'][c])
    return info, states, words


def decode(buf: bytes) -> np.ndarray:
    """The symbols of a stream; ValueError where a lane wants a word beyond its chunk, a final state is not 2^16 or a
    chunk's cursor does not end at its last word.  Word indices are clamped to the chunk before the read."""
    info, x, words = split(buf)
    n, R, f, nw = info['n'], info['R'], info['f'], info['words']
    nc = nw.size
    if n == 0:
        return np.zeros(0, np.uint8)
    cum = _cum(f)
    tab = np.repeat(np.arange(256), f)
    flat = np.concatenate(words + [np.zeros(1, np.int64)])
    starts = np.concatenate([[0], np.cumsum(nw)])[:nc]
    act = (np.arange(nc * 64 * R) < n).reshape(nc, R, 64)
    out = np.zeros((nc, R, 64), np.uint8)
    cursor = np.zeros(nc, np.int64)
    bad = False
    for r in range(R):
        a = act[:, r]
        slot = x & (M - 1)
        s = tab[slot]
        x = np.where(a, f[s] * (x >> M_BITS) + slot - cum[s], x)
        out[:, r] = s
        need = a & (x < LOW)
        idx = cursor[:, None] + np.cumsum(need, 1) - need
        bad |= bool((need & (idx >= nw[:, None])).any())
        idx = np.clip(idx, 0, np.maximum(nw - 1, 0)[:, None])
        w = np.where(nw[:, None] > 0, flat[starts[:, None] + idx], 0)
        x = np.where(need, (x << 16) | w, x)
        cursor += need.sum(1)
    if bad or np.any(x != LOW) or np.any(cursor != nw):
        raise ValueError('malformed rANS stream')
    return out.reshape(-1)[:n]


# ---- entropy-mode files ------------------------------------------------------------------------------------------------------

def plain_rest(labels: np.ndarray, bits: int) -> bytes:
    """What follows the centres in a plain block: the labels `bits` wide, MSB first, tail left-aligned, plus the uint32 last
    label when bits % 8 is non-zero."""
    labels = np.asarray(labels, np.int64)
    w = (labels[:, None] >> np.arange(bits - 1, -1, -1)[None, :]) & 1
    out = np.packbits(w.reshape(-1).astype(np.uint8)).tobytes()
    if bits % 8:
        out += struct.pack('<I', int(labels[-1]))
    return out


def label_streams(labels: np.ndarray, bits: int, R: int = ROUNDS) -> bytes:
    labels = np.asarray(labels, np.int64)
    if bits <= 8:
        return encode(labels.astype(np.uint8), R)
    return encode((labels & 0xFF).astype(np.uint8), R) + encode((labels >> 8).astype(np.uint8), R)


def coded(plain: bytes, stream: bytes) -> bytes:
    """[u8 mode][payload]: mode 1 only where the stream is strictly smaller."""
    return b'\x01' + stream if len(stream) < len(plain) else b'\x00' + plain


def write_files(header: dict, weights, biases, blocks, mask, R: int = ROUNDS) -> Tuple[bytes, bytes, List[int]]:
    """(parameter file, mask file, modes: one per block, then the mask's) for codebooks given as in ref_codec.serialize."""
    h = header
    bits = h['bit_precision']
    out = bytearray(struct.pack('9B', h['n_layers'], h['layer_width'], h['input_dim'], h['input_channel'], h['output_dim'],
                                bits | 0x80, h['grid_size'], h['n_grids'], h['feature_size']))
    for v in list(h['grid_sizes']) + list(h['zeros']):
        out += struct.pack('<I', v)
    modes = []

    def put_floats(a):
        out.extend(np.asarray(a, dtype='<f4').tobytes())

    def put_block(b):
        put_floats(b['centres'])
        body = coded(plain_rest(b['labels'], bits), label_streams(b['labels'], bits, R))
        modes.append(body[0])
        out.extend(body)

    it = iter(blocks)
    put_floats(weights[0]); put_floats(biases[0])
    for i in range(1, h['n_layers']):
        put_block(next(it))
        put_floats(biases[i])
    put_floats(weights[-1]); put_floats(biases[-1])
    for _ in range(h['n_grids']):
        put_block(next(it))
    plain_mask = np.packbits(np.asarray(mask, dtype=np.uint8)).tobytes()
    mask_file = coded(plain_mask, encode(np.frombuffer(plain_mask, np.uint8), R))
    modes.append(mask_file[0])
    return bytes(out), mask_file, modes


def parse_files(param_file: bytes, mask_file: bytes) -> Dict[str, object]:
    """ref_codec.parse for an entropy-mode pair, plus 'modes' (one per block, then the mask's)."""
    pos = 0

    def take(fmt):
        nonlocal pos
        vals = struct.unpack_from(fmt, param_file, pos)
        pos += struct.calcsize(fmt)
        return vals

    n_layers, layer_width, input_dim, input_channel, output_dim, flag, grid_size, n_grids, feature_size = take('9B')
    assert flag & 0x80, 'not an entropy-mode file'
    bits = flag & 0x7F
    grid_sizes = [take('<I')[0] for _ in range(n_grids)]
    zeros = [take('<I')[0] for _ in range(n_grids)]
    blocks, modes = [], []

    def floats(n):
        return np.asarray(take('<%df' % n), dtype=np.float32)

    def plane():
        nonlocal pos
        info = stream_info(param_file, pos)
        sym = decode(param_file[pos:pos + info['nbytes']])
        pos += info['nbytes']
        return sym.astype(np.int64), info['f']

    def quantised(n):
        nonlocal pos
        centres = floats(1 << bits)
        mode = take('B')[0]
        modes.append(mode)
        if mode == 0:
            nbytes = (n * bits + 7) // 8
            labels = K.unpack_labels(param_file[pos:pos + nbytes], n, bits)
            pos += nbytes
            if bits % 8:
                labels[-1] = take('<I')[0]
        else:
            assert mode == 1
            labels, f = plane()
            assert not f[1 << min(bits, 8):].any()
            if bits > 8:
                hi, f = plane()
                assert not f[1 << (bits - 8):].any()
                labels = labels | (hi << 8)
            assert labels.size == n
        blocks.append({'centres': centres, 'labels': labels})
        return centres[labels]

    weights = [floats(input_dim * layer_width)]
    biases = [floats(layer_width)]
    for _ in range(n_layers - 1):
        weights.append(quantised(layer_width * layer_width))
        biases.append(floats(layer_width))
    weights.append(floats(output_dim * layer_width))
    biases.append(floats(output_dim))
    total = sum(grid_sizes) + sum(zeros)
    mask_bytes = mask_file[1:] if mask_file[0] == 0 else decode(mask_file[1:]).tobytes()
    modes_mask = mask_file[0]
    mask = np.unpackbits(np.frombuffer(mask_bytes, dtype=np.uint8))[:total].astype(bool)
    grids, at = [], 0
    for nz, z in zip(grid_sizes, zeros):
        vals = quantised(nz)
        full = np.zeros(nz + z, np.float32)
        full[mask[at:at + nz + z]] = vals
        at += nz + z
        grids.append(full)
    assert pos == len(param_file), 'trailing bytes in the parameter file'
    return {'header': dict(n_layers=n_layers, layer_width=layer_width, input_dim=input_dim, input_channel=input_channel,
                           output_dim=output_dim, bit_precision=bits, grid_size=grid_size, n_grids=n_grids,
                           feature_size=feature_size, grid_sizes=grid_sizes, zeros=zeros),
            'weights': weights, 'biases': biases, 'grids': grids, 'mask': mask, 'blocks': blocks,
            'modes': modes + [modes_mask]}
