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

import os
import re
import struct
from types import SimpleNamespace

import numpy as np
import torch

from .. import ops
from ..wavelet_transform.Torch_Wavelet_Transform import WaveletFilter3d
from .codec_container import Reader, read_field, write_field
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
    return _f32_bytes(centres) + write_field(rest, _label_streams(labels, bits))


_CHANNEL_MASK_MODE = 2    # first byte of a mask file that holds the mask once per cell: support + residual


def _channel_mask_file(grids, channels: int) -> bytes:
    """Mode 2 of the mask file: ``[u8 2][u32 K per tensor][field support][field residual]``.  A tensor is
    viewed as (channels, S cells); the support has one bit per cell (any channel non-zero), the residual the mask bits of the
    K support cells only, channel-major; a field is ``write_field`` over its MSB-first bytes."""
    flags = [ops.codec_support(g, channels) for g in grids]
    cells = [ops.codec_compact_support(g, channels, f) for g, f in zip(grids, flags)]
    support = ops.codec_pack_flags(torch.cat(flags))
    residual = ops.codec_mask(torch.cat([v.reshape(-1) for v in cells]))
    out = bytes([_CHANNEL_MASK_MODE]) + b''.join(struct.pack('<I', v.shape[1]) for v in cells)
    for field in (support, residual):
        out += write_field(field.cpu().numpy().tobytes(), [ops.codec_rans_encode(field)])
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
    mask_file = write_field(plain_mask, [ops.codec_rans_encode(mask)]) if entropy else plain_mask
    channels = int(model.feature_grid[0].shape[0])
    if channel_mask and all(g.numel() % channels == 0 for g in grids):
        per_cell = _channel_mask_file(grids, channels)
        if len(per_cell) < len(mask_file):
            mask_file = per_cell
    with open(filename + '_mask.bnr', 'wb') as f:
        f.write(mask_file)


def _parse_block(r: Reader, n: int, bits: int, entropy: bool) -> SimpleNamespace:
    """One quantised block of ``n`` labels: ``n, centres, mode`` and, mode 0, ``packed`` labels + ``last`` (the uint32 the
    writer repeats the last label in when bits % 8 != 0, reference :184-186, :265-267; else None) or, mode 1, ``planes``:
    (bytes, stream header) of the labels' low bytes and, above 8 bits, of their high bytes."""
    block = SimpleNamespace(n=n, centres=r.array('<f4', 1 << bits), packed=None, last=None, planes=None)
    nbytes, tail = (n * bits + 7) // 8, 4 if bits % 8 else 0
    streams = [(n, 1 << bits)] if bits <= 8 else [(n, 256), (n, 1 << (bits - 8))]
    block.mode, payload = read_field(r, nbytes + tail, streams, coded=entropy)
    if block.mode == 0:
        block.packed = payload[:nbytes]
        block.last = struct.unpack_from('<I', payload, nbytes)[0] if tail else None
    else:
        block.planes = payload
    return block


def _parse_mask(d: SimpleNamespace, mask_raw, what: str) -> SimpleNamespace:
    """``fields`` as ``read_field`` returns them, and ``cells``, ``kept``.  The flat mask (the plain file, or one field over
    all coefficients) has one field and None for the rest; a file that starts with byte 2 holds the mask once per cell:
    cells S_t and support cells K_t per tensor, then the support and the residual field."""
    r, total = Reader(mask_raw, what), sum(d.grid_sizes) + sum(d.zeros)
    if not d.entropy or bytes(r.view[:1]) != bytes([_CHANNEL_MASK_MODE]):
        field = read_field(r, None, [((total + 7) // 8, 256)], coded=d.entropy, exact=True)
        if field[0] == 0 and 8 * len(field[1]) < total:      # a longer plain mask is accepted, as by the reference
            raise ValueError('%s: %d bits needed, %d present' % (what, total, 8 * len(field[1])))
        return SimpleNamespace(fields=[field], cells=None, kept=None)
    C = d.feature_size
    if C < 1 or any((nz + z) % C for nz, z in zip(d.grid_sizes, d.zeros)):
        raise ValueError('%s: a tensor is no whole number of cells of %d channels' % (what, C))
    cells = [(nz + z) // C for nz, z in zip(d.grid_sizes, d.zeros)]
    kept = list(r.take('<B%dI' % d.n_grids)[1:])
    for t, (nz, S, K) in enumerate(zip(d.grid_sizes, cells, kept)):
        if K > S or nz > C * K:
            raise ValueError('%s: tensor %d has %d cells and %d non-zero coefficients, the file names %d support cells'
                             % (what, t, S, nz, K))
    fields = [read_field(r, (nbits + 7) // 8, [((nbits + 7) // 8, 256)]) for nbits in (sum(cells), C * sum(kept))]
    r.end()
    return SimpleNamespace(fields=fields, cells=cells, kept=kept)


def parse_model_files(raw, mask_raw, name: str = '') -> SimpleNamespace:
    """Host description of a parameter file and its mask file (bytes-like; ``name``: the parameter file's, for messages);
    nothing touches the GPU and no payload is copied.  ``n_layers, layer_width, input_dim, input_channel, output_dim, bits,
    entropy`` (header byte 5 split into the width and its 0x80 flag), ``grid_size, n_grids, feature_size``, ``grid_sizes``,
    ``zeros``; ``weights`` and ``biases`` per layer, fp32 arrays except the hidden weights, which like ``grid_blocks`` are
    blocks (``_parse_block``); ``mask`` (``_parse_mask``).  ValueError for a truncated file, a width outside 1..16, a field
    mode above 1, a stream header that does not add up, holds another number of symbols than its field or gives a
    frequency to a label the codebook does not have, a flat mask with too few bits or a stream that does not end with the
    file; in a per-cell mask file also trailing bytes, tensors that are no whole number of cells, more support cells than
    cells, and more non-zero coefficients than the support cells hold."""
    r = Reader(raw, name or 'parameter file')
    d = SimpleNamespace()
    d.n_layers, d.layer_width, d.input_dim, d.input_channel, d.output_dim, bits, d.grid_size, d.n_grids, d.feature_size = \
        r.take('9B')
    d.entropy, d.bits = bool(bits & _ENTROPY_FLAG), bits & ~_ENTROPY_FLAG
    if not 1 <= d.bits <= 16:
        raise ValueError('%s: bit precision %d not supported' % (r.what, d.bits))
    d.grid_sizes = list(r.take('<%dI' % d.n_grids))
    d.zeros = list(r.take('<%dI' % d.n_grids))
    d.weights, d.biases = [r.array('<f4', d.input_dim * d.layer_width)], [r.array('<f4', d.layer_width)]
    for _ in range(d.n_layers - 1):
        d.weights.append(_parse_block(r, d.layer_width * d.layer_width, d.bits, d.entropy))
        d.biases.append(r.array('<f4', d.layer_width))
    d.weights.append(r.array('<f4', d.output_dim * d.layer_width))
    d.biases.append(r.array('<f4', d.output_dim))
    d.grid_blocks = [_parse_block(r, nz, d.bits, d.entropy) for nz in d.grid_sizes]     # bytes after them are not looked at
    d.mask = _parse_mask(d, mask_raw, name + '_mask.bnr' if name else 'mask file')
    return d


def _upload(a, dev) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(dev)


def _field_on_device(field, dev) -> torch.Tensor:
    """The bytes of a one-stream field: uploaded as they are, or decoded."""
    mode, payload = field
    return _upload(payload, dev) if mode == 0 else ops.codec_rans_decode_parsed(_upload(payload[0][0], dev), payload[0][1])


def _dequantised(block: SimpleNamespace, bits: int, dev) -> torch.Tensor:
    n, centres = block.n, _upload(block.centres, dev)
    if n == 0:
        return torch.empty(0, device=dev)
    if block.mode == 0:
        out = ops.codec_dequant(_upload(block.packed, dev), bits, n, centres)
        if block.last is not None:
            out[-1] = centres[block.last]
        return out
    # labels held as bytes are a bits = 8 stream, two planes interleaved high byte first a bits = 16 stream; the codebook
    # is padded to that width (the host's frequency check keeps every label below 2^bits)
    planes = [ops.codec_rans_decode_parsed(_upload(data, dev), info) for data, info in block.planes]
    width = 8 * len(planes)
    packed = planes[0] if len(planes) == 1 else torch.stack([planes[1], planes[0]], dim=1).reshape(-1)
    padded = torch.zeros(1 << width, dtype=torch.float32, device=dev)
    padded[:1 << bits] = centres
    return ops.codec_dequant(packed, width, n, padded)


def _expand_flat(d: SimpleNamespace, dev) -> list:
    """Every coefficient tensor, flat: its values at the set bits of the flat mask."""
    mask, grids, bit_offset = _field_on_device(d.mask.fields[0], dev), [], 0
    for block, nz, z in zip(d.grid_blocks, d.grid_sizes, d.zeros):
        grids.append(ops.codec_expand(mask, bit_offset, nz + z, _dequantised(block, d.bits, dev)))
        bit_offset += nz + z
    return grids


def _expand_per_cell(d: SimpleNamespace, what: str, dev) -> list:
    """The same from a per-cell mask: the values go to the set residual bits of the tensor's support cells, the cells to
    the set support bits.  The values are padded to the residual range's length, so no residual makes the expansion read
    past them; the two counts the host could not check -- set residual bits = non-zero coefficients, set support bits = K
    -- come back from the device once, after the last tensor."""
    support, residual = [_field_on_device(f, dev) for f in d.mask.fields]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    grids, found, cell_offset, bit_offset = [], [], 0, 0
    for block, nz, S, K in zip(d.grid_blocks, d.grid_sizes, d.mask.cells, d.mask.kept):
        n = d.feature_size * K
        values = torch.zeros(n, dtype=torch.float32, device=dev)
        if n:
            values[:nz] = _dequantised(block, d.bits, dev)
            values, count = ops.codec_expand(residual, bit_offset, n, values, counted=True)
            found.append(count)
        else:
            found.append(torch.zeros((), dtype=torch.int64, device=dev))
        grids.append(ops.codec_expand_support(support, cell_offset, d.feature_size, S, values, K, status))
        cell_offset += S
        bit_offset += n
    found = torch.stack(found).cpu().tolist()
    if int(status.item()) or found != d.grid_sizes:
        raise ValueError('%s: the support or the residual does not hold the number of set bits the files name (support cells '
                         '%s, status %d; non-zero coefficients %s, set residual bits %s)'
                         % (what, d.mask.kept, int(status.item()), d.grid_sizes, found))
    return grids


def _decode_model_files(d: SimpleNamespace, name: str):
    """(weights, biases, flat coefficient tensors) of a parsed pair, on the GPU: all the per-coefficient work."""
    dev = torch.device('cuda')
    weights = [_upload(w, dev) if isinstance(w, np.ndarray) else _dequantised(w, d.bits, dev) for w in d.weights]
    biases = [_upload(b, dev) for b in d.biases]
    grids = _expand_flat(d, dev) if d.mask.cells is None else _expand_per_cell(d, name + '_mask.bnr', dev)
    return weights, biases, grids


def restore_model(filename, wavelet_filter='db2'):
    """Rebuild the model a parameter file + mask file describe (reference :226-332).  Like the reference the network is
    re-created with 'fourier' embedding (2 frequencies) and no drop layers; unlike it the model is returned on the GPU
    (it cannot run anywhere else).  The format has no field for the wavelet basis: ``wavelet_filter`` (passed on to
    ``setup_model``) names the one the stored model was built with, db2 like the reference by default.

    Every kind of pair ``store_model_parameters`` writes is recognised from the files themselves, and read and checked on the
    host in full (``parse_model_files``: ValueError) before the first device call.  The two counts of a per-cell mask that
    only the device can check -- set support bits and set residual bits per tensor -- raise ``ValueError`` after the
    expansion, which is made safe against either being wrong."""
    with open(filename, 'rb') as f:
        raw = f.read()
    with open(filename + '_mask.bnr', 'rb') as f:
        mask_raw = f.read()
    d = parse_model_files(raw, mask_raw, filename)
    net_weights, net_biases, grid_params = _decode_model_files(d, filename)
    model = setup_model(input_channel=d.input_channel, hidden_channel=d.layer_width, out_channel=d.output_dim,
                        num_layer=d.n_layers, embedding_type='fourier', n_embedding_freq=2, drop_type='',
                        drop_momentum=0.025, drop_threshold=0.75, wavelet_filter=wavelet_filter,
                        grid_features=d.feature_size, grid_size=d.grid_size, checkpoint_path='').to('cuda')
    built = [p.numel() for name, p in model.named_parameters() if re.match(r'.*grid.*', name, re.I)]
    stored = [nz + z for nz, z in zip(d.grid_sizes, d.zeros)]
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
