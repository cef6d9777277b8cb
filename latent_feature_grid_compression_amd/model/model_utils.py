"""Counterpart of model/model_utils.py: ``setup_model`` (:23-59, the constructor call site of the hot path) and the
binary checkpoint codec ``store_model_parameters`` / ``restore_model`` (:120-332) with the same signatures and the SAME
FILE FORMAT, so files written by either implementation are read by the other.

The reference's codec does its per-coefficient work in Python (mask string concatenation :207-208, one ``np.insert``
per pruned coefficient :302-305, scikit-learn k-means on the host) and is unusable beyond toy sizes; here that work runs
on the GPU through the C-ABI (``lfgc_codec_*``: bit mask, order-preserving compaction / expansion, 1-D k-means, label
dequantisation) and only the file layout itself (header, layer fields, byte streams) is host code below.

``store_model_parameters(..., entropy=True)`` is this package's own extension: a lossless rANS stage over the labels and the
mask (``lfgc_codec_rans_*``), flagged in the header so that the reference's reader refuses such a file
instead of misreading it.  Without it the files are the reference's.  ``channel_mask=True`` on top of it lets the mask file
store the pruning pattern once per cell instead of once per coefficient (``lfgc_codec_support_f32`` and its companions).
"""
from __future__ import annotations

import math
import os
import re
import struct

import numpy as np
import torch

from .. import ops

from ..wavelet_transform.Torch_Wavelet_Transform import WaveletFilter3d
from .Feature_Embedding import FourierEmbedding
from .Feature_Grid_Model import Feature_Grid_Model
from .Smallify_Dropout import SmallifyDropout
from .Straight_Through_Dropout import MaskedWavelet_Straight_Through_Dropout, Straight_Through_Dropout
from .Variational_Dropout_Layer import VariationalDropout


def setup_model(input_channel, hidden_channel, out_channel, num_layer, embedding_type, n_embedding_freq, drop_type,
                drop_momentum, drop_threshold, wavelet_filter, grid_features, grid_size, checkpoint_path,
                drop_layer=None, num_levels=None):
    """Same positional arguments as the reference (``drop_type``: '' | 'smallify' | 'straight_through' |
    'masked_straight_through' | anything containing 'variational', reference :35-45).  Extras: ``drop_layer`` = a
    ready prototype object with the DropoutLayer interface (takes precedence), ``num_levels`` = wavelet depth."""
    size_tensor = (grid_features, grid_size, grid_size, grid_size)
    feature_grid = torch.empty(size_tensor).uniform_(0, 1)
    wavelet = WaveletFilter3d(wavelet_filter)
    if drop_type and drop_layer is None:
        size = feature_grid.shape[1:]
        if drop_type == 'smallify':
            drop_layer = SmallifyDropout(size, drop_momentum, drop_threshold)
        if drop_type == 'straight_through':
            drop_layer = Straight_Through_Dropout(size, drop_momentum, drop_threshold)
        if drop_type == 'masked_straight_through':
            drop_layer = MaskedWavelet_Straight_Through_Dropout(size, drop_momentum, drop_threshold)
        if 'variational' in drop_type:
            drop_layer = VariationalDropout(size, drop_momentum, drop_threshold)
        if drop_layer is None:
            raise ValueError('unknown drop_type %r' % (drop_type,))
    embedder = FourierEmbedding(n_freqs=n_embedding_freq, input_dim=input_channel)
    model = Feature_Grid_Model(embedder, feature_grid, drop_layer, wavelet, input_channel_data=input_channel,
                               hidden_channel=hidden_channel, out_channel=out_channel, num_layer=num_layer,
                               num_levels=num_levels)
    if checkpoint_path:
        model.load_state_dict(torch.load(checkpoint_path, weights_only=True))
    return model


def write_dict(dictionary, filename, experiment_path=''):
    with open(os.path.join(experiment_path, filename), 'w') as f:
        for key, value in dictionary.items():
            f.write('%s = %s\n' % (key, value))


def get_net_weights_biases(net):
    """Parameters whose names end in .weight / .bias, in named_parameters() order (reference :62-70)."""
    weights = [p.data for name, p in net.named_parameters() if name.endswith('.weight')]
    biases = [p.data for name, p in net.named_parameters() if name.endswith('.bias')]
    return weights, biases


def kmeans_quantization(w, q):
    """(labels, centres) as Python lists like the reference helper (:73-76), ``q`` up to 65 536; the clustering runs on the
    GPU."""
    t = torch.as_tensor(np.asarray(w, dtype=np.float32).reshape(-1))
    centres, labels = ops.codec_kmeans(t.cuda(), int(q))
    return labels.cpu().numpy().tolist(), centres.cpu().tolist()


_BIT_PRECISION = 8        # the writer's default width: the only one the reference's own writer emits (:141)


def _check_bit_precision(bit_precision) -> int:
    if isinstance(bit_precision, bool) or not isinstance(bit_precision, (int, np.integer)) or not 1 <= bit_precision <= 16:
        raise ValueError('bit_precision must be an integer from 1 to 16, got %r' % (bit_precision,))
    return int(bit_precision)


def _device_flat(t: torch.Tensor) -> torch.Tensor:
    if not torch.cuda.is_available():
        raise ops._lib.LfgcError('the checkpoint codec runs its per-coefficient work on the MI355X: no GPU is visible. '
                                 'There is no CPU fallback.')
    return t.detach().to('cuda', torch.float32).reshape(-1)


def _f32_bytes(t) -> bytes:
    return np.ascontiguousarray(t.detach().cpu().numpy().reshape(-1).astype('<f4')).tobytes()


_ENTROPY_FLAG = 0x80      # header byte 5 of an entropy-mode file is bits | 0x80: older readers refuse it as a width


def _coded(plain: bytes, streams) -> bytes:
    """[u8 mode][payload] of an entropy-mode file: mode 1 and the rANS streams where they are strictly smaller than the plain
    bytes, else mode 0 and the plain bytes -- a field never grows by more than this one byte."""
    if sum(s.numel() for s in streams) < len(plain):
        return b'\x01' + b''.join(s.cpu().numpy().tobytes() for s in streams)
    return b'\x00' + plain


def _label_streams(labels: torch.Tensor, bits: int):
    """One rANS stream over the labels as bytes, or above 8 bits two: the plane label & 0xFF, then label >> 8."""
    if bits <= 8:
        return [ops.codec_rans_encode(labels)]
    wide = labels.to(torch.int32)
    return [ops.codec_rans_encode((wide & 0xFF).to(torch.uint8)), ops.codec_rans_encode((wide >> 8).to(torch.uint8))]


def _quantised_block(values: torch.Tensor, bits: int, entropy: bool = False) -> bytes:
    """[2^bits fp32 centres][labels, `bits` each, MSB first][bits % 8: the last label as uint32] (reference
    write_tensor_quantized :170-182).  At 8 bits the uint8 label array is the stream; at any other width
    lfgc_codec_pack_labels packs it, a partial last byte LEFT-aligned (include/lfgc.h) -- what the readers slice.
    ``entropy``: [centres][u8 mode] and then that same remainder (mode 0) or the labels' rANS streams (mode 1)."""
    centres, labels = ops.codec_kmeans(values, 1 << bits)
    if bits == 8:
        rest = labels.cpu().numpy().tobytes()
    else:
        rest = ops.codec_pack_labels(labels, bits).cpu().numpy().tobytes()
        if bits % 8 != 0:
            rest += struct.pack('<I', int(labels[-1:].cpu().numpy()[0]))
    if not entropy:
        return _f32_bytes(centres) + rest
    return _f32_bytes(centres) + _coded(rest, _label_streams(labels, bits))


_CHANNEL_MASK_MODE = 2    # first byte of a mask file that holds the mask once per cell: support + residual


def _channel_mask_file(grids, channels: int) -> bytes:
    """Mode 2 of the mask file: ``[u8 2][u32 K per tensor][field support][field residual]``.  A tensor is
    viewed as (channels, S cells); the support has one bit per cell (any channel non-zero), the residual the mask bits of the
    K support cells only, channel-major; a field is ``_coded`` over its MSB-first bytes."""
    flags = [ops.codec_support(g, channels) for g in grids]
    cells = [ops.codec_compact_support(g, channels, f) for g, f in zip(grids, flags)]
    support = ops.codec_pack_flags(torch.cat(flags))
    residual = ops.codec_mask(torch.cat([v.reshape(-1) for v in cells]))
    out = bytes([_CHANNEL_MASK_MODE]) + b''.join(struct.pack('<I', v.shape[1]) for v in cells)
    for field in (support, residual):
        out += _coded(field.cpu().numpy().tobytes(), [ops.codec_rans_encode(field)])
    return out


def store_model_parameters(model, filename, bit_precision=_BIT_PRECISION, entropy=False, channel_mask=False):
    """Write ``filename`` (header, first / final layer in fp32, hidden layers and the non-zero wavelet coefficients as
    ``bit_precision``-bit codebook indices, 1 to 16) and ``filename + "_mask.bnr"`` (bit mask of the non-zero
    coefficients): reference :120-223, whose ``bit_precision = 8`` (:141) is the default here.

    ``entropy=True`` adds the lossless rANS stage: header byte 5 becomes ``bits | 0x80``, every quantised
    block is ``[centres][u8 mode]`` + the plain remainder (mode 0) or the labels' rANS streams (mode 1), and the mask file is
    ``[u8 mode]`` + the plain mask or its rANS stream; mode 1 only where it is strictly smaller.  ``restore_model`` reads
    either kind.  The default writes the same bytes as before.

    ``channel_mask=True`` (needs ``entropy=True``: the plain mask file has no mode byte) lets the mask file take a third
    mode, the mask once per cell: every drop layer prunes whole cells, so the zero pattern of a pruned model repeats in all
    channels, and mode 2 stores one support bit per cell plus the mask bits of the support cells only.  The writer forms
    modes 0, 1 and 2 and keeps the strictly smallest (ties: the lower mode), so a dense or per-coefficient-pruned model
    keeps the ``entropy=True`` file; the parameter file is the ``entropy=True`` one, byte for byte.  ``restore_model``
    recognises the mode from the mask file's first byte."""
    bits = _check_bit_precision(bit_precision)
    entropy, channel_mask = bool(entropy), bool(channel_mask)
    if channel_mask and not entropy:
        raise ValueError('channel_mask=True needs entropy=True: the plain mask file has no mode byte')
    if len(model.shape_array) == 0:
        raise ValueError('a model without wavelet levels has no grid_size to put in the header (reference :131)')
    grids = [_device_flat(g) for g in model.feature_grid]
    nonzero = [ops.codec_compact(g) for g in grids]
    header = struct.pack('9B', model.num_layer, model.hidden_width, model.input_channel, model.d_in, model.output_channel,
                         bits | (_ENTROPY_FLAG if entropy else 0), int(model.shape_array[-1][0]), len(grids),
                         int(model.feature_grid[0].shape[0]))
    weights, biases = get_net_weights_biases(model)
    with open(filename, 'wb') as f:
        f.write(header)
        for g, nz in zip(grids, nonzero):
            f.write(struct.pack('<I', nz.numel()))
        for g, nz in zip(grids, nonzero):
            f.write(struct.pack('<I', g.numel() - nz.numel()))
        f.write(_f32_bytes(weights[0]))
        f.write(_f32_bytes(biases[0]))
        for w, b in zip(weights[1:-1], biases[1:-1]):
            f.write(_quantised_block(_device_flat(w), bits, entropy))
            f.write(_f32_bytes(b))
        f.write(_f32_bytes(weights[-1]))
        f.write(_f32_bytes(biases[-1]))
        for nz in nonzero:
            if nz.numel() == 0:
                raise ValueError('a coefficient tensor without any non-zero entry cannot be quantised (the reference '
                                 'fails in KMeans here as well)')
            f.write(_quantised_block(nz, bits, entropy))
    mask = ops.codec_mask(torch.cat(grids))           # one bit stream over all tensors, like the reference's mask_string
    plain_mask = mask.cpu().numpy().tobytes()
    mask_file = _coded(plain_mask, [ops.codec_rans_encode(mask)]) if entropy else plain_mask
    channels = int(model.feature_grid[0].shape[0])
    if channel_mask and all(g.numel() % channels == 0 for g in grids):
        per_cell = _channel_mask_file(grids, channels)
        if len(per_cell) < len(mask_file):
            mask_file = per_cell
    with open(filename + '_mask.bnr', 'wb') as f:
        f.write(mask_file)


def restore_model(filename, wavelet_filter='db2'):
    """Rebuild the model a parameter file + mask file describe (reference :226-332).  Like the reference the network is
    re-created with 'fourier' embedding (2 frequencies) and no drop layers; unlike it the model is returned on the GPU
    (it cannot run anywhere else).  The format has no field for the wavelet basis: ``wavelet_filter`` (passed on to
    ``setup_model``) names the one the stored model was built with, db2 like the reference by default.

    An entropy-mode pair (``store_model_parameters(..., entropy=True)``) is recognised by header byte 5 (``bits | 0x80``).
    Both kinds are read and checked on the host in full -- ``ValueError`` for a truncated file, a stream header that does
    not add up, or a frequency on a label the codebook does not have -- before the first device call.

    A mask file in mode 2 (``channel_mask=True``: the mask once per cell) is recognised by its first byte.
    Its host checks: truncation, trailing bytes, a field mode above 1, tensors that are no whole number of cells, more
    support cells than cells, more non-zero coefficients than the support cells hold, a stream of another length than its
    field.  The two counts only the device can check -- set support bits and set residual bits per tensor -- raise
    ``ValueError`` after the expansion, which is made safe against either being wrong."""
    with open(filename, 'rb') as f:
        raw = f.read()
    with open(filename + '_mask.bnr', 'rb') as f:
        mask_raw = f.read()
    pos = 0

    # ---- 1. the whole file pair is read and checked on the host, before anything touches the GPU --------------------
    def take(fmt):
        nonlocal pos
        size = struct.calcsize(fmt)
        if pos + size > len(raw):
            raise ValueError('%s: truncated parameter file' % filename)
        vals = struct.unpack(fmt, raw[pos:pos + size])
        pos += size
        return vals

    n_layers, layer_width, input_dim, input_channel, output_dim, bits, grid_size, n_grids, feature_size = take('9B')
    entropy = bool(bits & _ENTROPY_FLAG)
    bits &= ~_ENTROPY_FLAG
    if not 1 <= bits <= 16:
        raise ValueError('%s: bit precision %d not supported' % (filename, bits))
    n_clusters = int(math.pow(2, bits))
    grid_sizes = [take('<I')[0] for _ in range(n_grids)]
    zeros = [take('<I')[0] for _ in range(n_grids)]

    def floats(n):
        nonlocal pos
        if pos + 4 * n > len(raw):
            raise ValueError('%s: truncated parameter file' % filename)
        a = np.frombuffer(raw, dtype='<f4', count=n, offset=pos)
        pos += 4 * n
        return torch.from_numpy(a.astype(np.float32))

    def rans_stream(buf, at, n, n_symbols, what, exact=False):
        """(bytes, header) of the rANS stream at buf[at:] that must hold n symbols below n_symbols."""
        try:
            info = ops.codec_rans_header(buf, at, exact=exact)
        except ValueError as e:
            raise ValueError('%s: %s' % (what, e)) from None
        if info.n != n:
            raise ValueError('%s: a stream of %d symbols where %d are expected' % (what, info.n, n))
        if info.freq[n_symbols:].any():          # a decoded label can then never index past the codebook
            raise ValueError('%s: the model gives a frequency to a symbol of %d or above' % (what, n_symbols))
        return np.frombuffer(buf, dtype=np.uint8, count=info.nbytes, offset=at), info

    def quantised(n):
        """Host description of one block: the centres, and the packed labels (+ the uint32 last label) or the rANS planes."""
        nonlocal pos
        block = {'n': n, 'centres': floats(n_clusters), 'last': None, 'packed': None, 'planes': None}
        mode = take('B')[0] if entropy else 0
        if mode == 0:
            nbytes = (n * bits) // 8 + (1 if (n * bits) % 8 else 0)
            if pos + nbytes > len(raw):
                raise ValueError('%s: truncated parameter file' % filename)
            block['packed'] = np.frombuffer(raw, dtype=np.uint8, count=nbytes, offset=pos)
            pos += nbytes
            if bits % 8 != 0:                   # the writer repeats the last label as a uint32 (:184-186, :265-267)
                block['last'] = take('<I')[0]
        elif mode == 1:
            block['planes'] = []
            for limit in ([1 << bits] if bits <= 8 else [256, 1 << (bits - 8)]):
                data, info = rans_stream(raw, pos, n, limit, filename)
                pos += info.nbytes
                block['planes'].append((data, info))
        else:
            raise ValueError('%s: block mode %d not supported' % (filename, mode))
        return block

    net_weights = [floats(input_dim * layer_width)]
    net_biases = [floats(layer_width)]
    for _ in range(n_layers - 1):
        net_weights.append(quantised(layer_width * layer_width))
        net_biases.append(floats(layer_width))
    net_weights.append(floats(output_dim * layer_width))
    net_biases.append(floats(output_dim))
    grid_blocks = [quantised(nz) for nz in grid_sizes]

    def per_cell_mask():
        """Host description of a mode-2 mask file: (cells S_t, support cells K_t, [(bytes, stream header or None) of the
        support and of the residual field])."""
        what = filename + '_mask.bnr'
        if feature_size < 1 or any((nz + z) % feature_size for nz, z in zip(grid_sizes, zeros)):
            raise ValueError('%s: a tensor is no whole number of cells of %d channels' % (what, feature_size))
        cells = [(nz + z) // feature_size for nz, z in zip(grid_sizes, zeros)]
        at = 1 + 4 * n_grids
        if len(mask_raw) < at:
            raise ValueError('%s: truncated mask file' % what)
        kept = list(struct.unpack_from('<%dI' % n_grids, mask_raw, 1))
        for t, (nz, S, K) in enumerate(zip(grid_sizes, cells, kept)):
            if K > S or nz > feature_size * K:
                raise ValueError('%s: tensor %d has %d cells and %d non-zero coefficients, the file names %d support cells'
                                 % (what, t, S, nz, K))
        fields = []
        for nbits in (sum(cells), feature_size * sum(kept)):
            nbytes = (nbits + 7) // 8
            if at >= len(mask_raw):
                raise ValueError('%s: truncated mask file' % what)
            mode = mask_raw[at]
            at += 1
            if mode == 0:
                if at + nbytes > len(mask_raw):
                    raise ValueError('%s: truncated mask file' % what)
                fields.append((np.frombuffer(mask_raw[at:at + nbytes], dtype=np.uint8), None))
                at += nbytes
            elif mode == 1:
                fields.append(rans_stream(mask_raw, at, nbytes, 256, what))
                at += fields[-1][1].nbytes
            else:
                raise ValueError('%s: field mode %d not supported' % (what, mode))
        if at != len(mask_raw):
            raise ValueError('%s: %d trailing bytes' % (what, len(mask_raw) - at))
        return cells, kept, fields

    total = sum(grid_sizes) + sum(zeros)
    mask_stream = per_cell = None
    if not entropy:
        mask_bytes = len(mask_raw)
    elif len(mask_raw) < 1 or mask_raw[0] > _CHANNEL_MASK_MODE:
        raise ValueError('%s_mask.bnr: %s' % (filename, 'mode %d not supported' % mask_raw[0] if mask_raw else 'empty'))
    elif mask_raw[0] == _CHANNEL_MASK_MODE:
        per_cell = per_cell_mask()
        mask_bytes = (total + 7) // 8            # the flat mask is never materialised
    elif mask_raw[0] == 0:
        mask_raw = mask_raw[1:]
        mask_bytes = len(mask_raw)
    else:
        mask_stream = rans_stream(mask_raw, 1, (total + 7) // 8, 256, filename + '_mask.bnr', exact=True)
        mask_bytes = mask_stream[1].n
    if mask_bytes * 8 < total:
        raise ValueError('%s_mask.bnr: %d bits needed, %d present' % (filename, total, mask_bytes * 8))

    # ---- 2. the per-coefficient work, on the GPU -------------------------------------------------------------------------
    dev = torch.device('cuda')

    def upload(a):
        return torch.from_numpy(np.array(a)).to(dev)

    def dequantised(block):
        n, centres = block['n'], block['centres'].to(dev)
        if n == 0:
            return torch.empty(0, device=dev)
        if block['planes'] is None:
            out = ops.codec_dequant(upload(block['packed']), bits, n, centres)
            if block['last'] is not None:
                out[-1] = centres[block['last']]
            return out
        # labels held as bytes are a bits = 8 stream, two planes interleaved high byte first a bits = 16 stream; the
        # codebook is padded to that width (the frequency check above keeps every label below 2^bits)
        planes = [ops.codec_rans_decode_parsed(upload(data), info) for data, info in block['planes']]
        width = 8 * len(planes)
        packed = planes[0] if len(planes) == 1 else torch.stack([planes[1], planes[0]], dim=1).reshape(-1)
        padded = torch.zeros(1 << width, dtype=torch.float32, device=dev)
        padded[:n_clusters] = centres
        return ops.codec_dequant(packed, width, n, padded)

    net_weights = [w.to(dev) if torch.is_tensor(w) else dequantised(w) for w in net_weights]
    net_biases = [b.to(dev) for b in net_biases]
    grid_params, bit_offset = [], 0
    if per_cell is not None:
        # mode 2: the values go to the set residual bits of the tensor's support cells, the cells to the set support bits.
        # The values are padded to the residual range's length, so no residual makes the expansion read past them; the
        # two counts the host could not check -- set residual bits = non-zero coefficients, set support bits = K -- come
        # back from the device once, after the last tensor.
        cells, kept, fields = per_cell
        support, residual = [upload(data) if info is None else ops.codec_rans_decode_parsed(upload(data), info)
                             for data, info in fields]
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        found, cell_offset = [], 0
        for block, nz, S, K in zip(grid_blocks, grid_sizes, cells, kept):
            n = feature_size * K
            values = torch.zeros(n, dtype=torch.float32, device=dev)
            if n:
                values[:nz] = dequantised(block)
                values, count = ops.codec_expand(residual, bit_offset, n, values, counted=True)
                found.append(count)
            else:
                found.append(torch.zeros((), dtype=torch.int64, device=dev))
            grid_params.append(ops.codec_expand_support(support, cell_offset, feature_size, S, values, K, status))
            cell_offset += S
            bit_offset += n
        found = torch.stack(found).cpu().tolist()
        if int(status.item()) or found != grid_sizes:
            raise ValueError('%s_mask.bnr: the support or the residual does not hold the number of set bits the files name '
                             '(support cells %s, status %d; non-zero coefficients %s, set residual bits %s)'
                             % (filename, kept, int(status.item()), grid_sizes, found))
    else:
        if mask_stream is None:
            mask = upload(np.frombuffer(mask_raw, dtype=np.uint8))
        else:
            mask = ops.codec_rans_decode_parsed(upload(mask_stream[0]), mask_stream[1])
        for block, nz, z in zip(grid_blocks, grid_sizes, zeros):
            grid_params.append(ops.codec_expand(mask, bit_offset, nz + z, dequantised(block)))
            bit_offset += nz + z

    model = setup_model(input_channel=input_channel, hidden_channel=layer_width, out_channel=output_dim,
                        num_layer=n_layers, embedding_type='fourier', n_embedding_freq=2, drop_type='',
                        drop_momentum=0.025, drop_threshold=0.75, wavelet_filter=wavelet_filter,
                        grid_features=feature_size, grid_size=grid_size, checkpoint_path='').to(dev)
    built = [p.numel() for name, p in model.named_parameters() if re.match(r'.*grid.*', name, re.I)]
    stored = [nz + z for nz, z in zip(grid_sizes, zeros)]
    if built != stored:
        raise ValueError('%s holds %d coefficient tensors of %s elements, a %r model of this shape has %d of %s: name the '
                         'stored model\'s basis with wavelet_filter=' % (filename, len(stored), stored, wavelet_filter,
                                                                        len(built), built))
    wdx = bdx = gdx = 0
    for name, p in model.named_parameters():        # same name tests, same order as the reference (:316-328)
        if re.match(r'.*grid.*', name, re.I):
            p.data = grid_params[gdx].view(p.data.shape)
            gdx += 1
        if re.match(r'.*.weight', name, re.I):
            p.data = net_weights[wdx].view(p.data.shape)
            wdx += 1
        if re.match(r'.*.bias', name, re.I):
            p.data = net_biases[bdx].view(p.data.shape)
            bdx += 1
    return model


# the error-bounded residual layer over a stored model is exported from here as well
from .residual_codec import PredictionMismatch, parse_residual_file, restore_volume, store_residuals  # noqa: E402,F401
