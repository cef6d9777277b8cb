"""The container layer under the checkpoint codec (model_utils.py) and the residual stream (residual_codec.py): a
bounds-checked cursor over a file's bytes, and the one field both formats are made of::

    field = [u8 mode][payload]     mode 0: the plain bytes     mode 1: their rANS stream(s), only where strictly smaller

Host code only: nothing here touches the GPU (``ops.codec_rans_header`` reads a stream's header on the host)."""
from __future__ import annotations

import struct

import numpy as np

from .. import ops


class Reader:
    """A cursor over ``raw`` (bytes-like) that never reads past its end; every failure is a ValueError that starts with
    ``what``, the file's name."""

    def __init__(self, raw, what: str):
        self.view, self.what, self.at = memoryview(raw).cast('B'), what, 0

    def room(self) -> int:
        return len(self.view) - self.at

    def _advance(self, size: int) -> int:
        if size > self.room():
            raise ValueError('%s: truncated: %d bytes needed at offset %d, %d are there' % (self.what, size, self.at, self.room()))
        self.at += size
        return self.at - size

    def take(self, fmt: str) -> tuple:
        return struct.unpack_from(fmt, self.view, self._advance(struct.calcsize(fmt)))

    def array(self, dtype, count: int) -> np.ndarray:
        """``count`` items as a view of the buffer: payloads of hundreds of MB are not copied."""
        return np.frombuffer(self.view, dtype, count, self._advance(np.dtype(dtype).itemsize * count))

    def stream(self, n: int, limit: int = 256, length=None, exact: bool = False):
        """(bytes, header) of the rANS stream here, which must hold ``n`` symbols, all below ``limit``, within ``length``
        bytes (default: the rest of the buffer; ``exact``: all of them)."""
        try:
            info = ops.codec_rans_header(self.view, self.at, length, exact=exact)
        except ValueError as e:
            raise ValueError('%s: %s' % (self.what, e)) from None
        if info.n != n:
            raise ValueError('%s: a stream of %d symbols where %d are expected' % (self.what, info.n, n))
        if info.freq[limit:].any():              # a decoded label can then never index past the codebook
            raise ValueError('%s: the model gives a frequency to a symbol of %d or above' % (self.what, limit))
        return self.array(np.uint8, info.nbytes), info

    def end(self) -> None:
        if self.room():
            raise ValueError('%s: %d trailing bytes' % (self.what, self.room()))


def write_field(plain: bytes, streams) -> bytes:
    """Mode 1 and the rANS streams (uint8 tensors) where they are strictly smaller than the plain bytes, else mode 0 and the
    plain bytes -- a field never grows by more than its mode byte."""
    if sum(s.numel() for s in streams) < len(plain):
        return b'\x01' + b''.join(s.cpu().numpy().tobytes() for s in streams)
    return b'\x00' + plain


def read_field(reader: Reader, plain_bytes, streams, coded: bool = True, **stream_kw):
    """(mode, payload) of the field at the cursor: in mode 0 the view of its ``plain_bytes`` bytes (None: the rest of the
    buffer), in mode 1 the list of ``Reader.stream(n, limit, **stream_kw)`` for the ``(n, limit)`` pairs of ``streams``.
    ``coded=False`` is the plain format: no mode byte, mode 0."""
    mode = reader.take('B')[0] if coded else 0
    if mode == 0:
        return 0, reader.array(np.uint8, reader.room() if plain_bytes is None else plain_bytes)
    if mode == 1:
        return 1, [reader.stream(n, limit, **stream_kw) for n, limit in streams]
    raise ValueError('%s: field mode %d not supported' % (reader.what, mode))
