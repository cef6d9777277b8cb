"""Drop-in for the reference's model/Feature_Grid_Model.py (class Feature_Grid_Model :16-140).

Same constructor, ``forward(input)`` signature, attribute names, parameter names/order and state_dict
keys, so it slots into Feature_Grid_Training.py / Feature_Grid_Inference.py in place of the original.
What differs is where the arithmetic runs: ``forward`` = HIP inverse-wavelet decode of the latent grid
(channel-last, cached while the parameters do not change in eval mode) + ONE fused HIP kernel for
trilinear sampling, Fourier embedding and the SnakeAlt MLP, with hand-written HIP backward kernels
behind ``torch.autograd.Function``.  There is no CPU path: a CPU tensor raises.
"""
from __future__ import annotations

import os
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..wavelet_transform.Torch_Wavelet_Transform import _WaveletFilterNd, dwt_max_level
from .Dropout_Layer import DropoutLayer
from .Feature_Embedding import Embedder


def SnakeAlt(x):
    return 0.5 * x + torch.sin(x) ** 2


class Feature_Grid_Model(nn.Module):
    def __init__(self, embedder: Embedder, feature_grid, drop_layer, wavelet_filter: _WaveletFilterNd,
                 input_channel_data=3, hidden_channel=32, out_channel=1, num_layer=4, num_levels=None):
        super().__init__()
        self.embedder = embedder
        self.filter = wavelet_filter

        features, shapes = self.encode_volume(feature_grid, num_levels=num_levels)
        # the reference keeps the detail bands as strided views of the encoder output (filtered[0, :, 1:]); stored
        # contiguous here (same values, same shapes) so the kernels bind them without a per-call copy
        self.feature_grid = nn.ParameterList([nn.Parameter(f.contiguous(), requires_grad=True) for f in features])
        self.shape_array = shapes

        if drop_layer is None:
            self.drop = nn.ModuleList([nn.Identity() for _ in features])
        else:
            self.drop = nn.ModuleList([drop_layer.create_instance(f.shape[1:], drop_layer.p, drop_layer.threshold)
                                       for f in features])

        self.input_channel = input_channel_data + embedder.out_dim + feature_grid.shape[0]
        self.hidden_width = hidden_channel
        self.output_channel = out_channel
        self.num_layer = num_layer
        self.d_in = input_channel_data
        self.grid_channels = int(feature_grid.shape[0])
        n_freqs = getattr(embedder, 'n_freqs', None)
        if n_freqs is None:
            n_freqs = embedder.out_dim // (2 * input_channel_data)
        self.n_freqs = int(n_freqs)

        self.net_layers = nn.ModuleList(
            [nn.Linear(self.input_channel, self.hidden_width)] +
            [nn.Linear(self.hidden_width, self.hidden_width) for _ in range(self.num_layer - 1)])
        self.final_layer = nn.Linear(self.hidden_width, self.output_channel)

        # arithmetic of the layer GEMMs: 'f16x2' (f16 hi+lo split, 3 MFMAs per product, fp32 accumulate: same error
        # level as fp32 against the reference, ~3x faster; a pass in which any sample leaves the f16 range -- |pre-
        # activation| >~ 800 or |grid feature| >= 65504, a diverged model -- is redone by the library on the exact build,
        # so the result is reference-equivalent for any finite parameters: include/lfgc.h, lfgc_forward_f32 `status`)
        # or 'fp32' (exact f32 MFMA throughout)
        self.precision = 'f16x2'
        # bitwise repeatable gradients (fixed-point grid-gradient scatter, one writer per drop-factor gradient address):
        # None follows torch.are_deterministic_algorithms_enabled(), True / False force the mode.  Promised for the same
        # build, shapes, precision and device
        self.deterministic = None
        self._grid_cache = None      # (key, channel-last dense grid) while parameters are unchanged (eval)
        self._pack_cache = None      # (key, packed MLP blob)
        self._penalty_cache = None   # penalty sums taken inside the last differentiable fused decode
        self._penalty_wanted = False  # set by the first pruning loss that asks for them (cached_penalties)
        self._decode_count = 0       # part of the cache key: optimizers may change parameters without bumping versions
        self._desc = None

    # ---- caches -------------------------------------------------------------------------------------------
    # Derived device data (decoded channel-last grid, packed MLP blob) is cached ONLY in eval mode, keyed on
    # (data_ptr, in-place version) of every source tensor, and dropped on every train()/eval() call.  In training mode
    # nothing is cached: torch's fused optimizers (Adam(fused=True)) update parameters WITHOUT bumping their version
    # counters (tools/microbench/adam_version.py), so a version key alone would serve stale weights after a step.
    @staticmethod
    def _key(tensors) -> tuple:
        return tuple((t.data_ptr(), t._version, t.device.index) for t in tensors)

    def invalidate_caches(self) -> None:
        """Forget every derived buffer.  Called by train()/eval(); call it yourself after changing parameters in eval
        mode through an op that does not bump tensor versions."""
        self._grid_cache = None
        self._pack_cache = None
        self._penalty_cache = None

    def train(self, mode: bool = True):
        self.invalidate_caches()
        return super().train(mode)

    def _mlp_params(self):
        layers = list(self.net_layers) + [self.final_layer]
        return [l.weight for l in layers], [l.bias for l in layers]

    def _descriptor(self):
        if self._desc is None:
            self._desc = ops.make_desc(self.grid_channels, self.hidden_width, self.num_layer, self.n_freqs,
                                       self.d_in, self.output_channel)
        return self._desc

    def _packed(self) -> torch.Tensor:
        weights, biases = self._mlp_params()
        if self.training:
            return ops.pack_mlp(self._descriptor(), weights, biases)
        key = self._key(weights + biases)
        if self._pack_cache is None or self._pack_cache[0] != key:
            self._pack_cache = (key, ops.pack_mlp(self._descriptor(), weights, biases))
        return self._pack_cache[1]

    def _identity_drop(self) -> bool:
        return all(isinstance(d, nn.Identity) for d in self.drop)

    def _dropped(self):
        """Coefficient tensors with their drop layers resolved (reference :103, :105): this package's layers only
        name their per-coefficient factor -- the multiply happens inside the IDWT kernels --, any other module
        (nn.Identity, a reference DropoutLayer object handed in by the caller) is called as it is."""
        coeffs, factors, thresholds, l1_flags = [], [], [], []
        DropoutLayer.prepare(self.drop)
        for g, d in zip(self.feature_grid, self.drop):
            f = d.drop_factor() if isinstance(d, DropoutLayer) else None
            if f is None and not isinstance(d, (nn.Identity, DropoutLayer)):
                g = d(g)
            coeffs.append(g)
            factors.append(None if f is None else f.mul)
            thresholds.append(None if f is None else f.threshold)
            l1_flags.append(bool(f is not None and f.l1_target))
        return coeffs, factors, thresholds, l1_flags

    def _penalty_key(self):
        """Identity + in-place version of every tensor the cached penalty sums were taken of."""
        ts = list(self.feature_grid) + [p for d in self.drop for p in d.parameters()]
        return tuple((id(t), t._version) for t in ts)

    def cached_penalties(self):
        """(sum of squared coefficients per tensor (n,), {drop-layer index: its L1 term}) from the last differentiable
        decode, with their gradients riding in that decode's backward kernels -- or None if no decode has run since a
        parameter last changed (the pruning losses then evaluate the terms with a launch of their own)."""
        # the sums are only produced once a loss has shown that it consumes them: the fine-tune phase of the reference
        # (training/training.py:236: drop_loss=None with the mask layers still installed) then pays no penalty launch
        self._penalty_wanted = True
        c, self._penalty_cache = self._penalty_cache, None      # consumed once: see _decode on why no reference is kept
        if c is None or c['key'] != self._penalty_key() or c['decode'] != self._decode_count or not torch.is_grad_enabled():
            return None
        n = c['n']
        l1 = {i: c['pen'][n + j] for j, i in enumerate(c['l1_idx'])}
        return c['pen'][:n], l1

    def _decode(self, channel_last: bool) -> torch.Tensor:
        coeffs, factors, thresholds, l1_flags = self._dropped()
        self._penalty_cache = None
        self._decode_count += 1
        fused = any(f is not None for f in factors)
        if fused and len(coeffs) == 1:                     # no wavelet level at all: the layer is all there is
            coeffs = [ops.DropApplyFn.apply(coeffs[0], factors[0], thresholds[0])]
            fused = False
        track = torch.is_grad_enabled() and any(t.requires_grad for t in coeffs + [f for f in factors if f is not None])
        if fused:
            if track:
                # penalty sums of the coefficients (and of factors that are themselves L1-penalised parameters) come
                # out of the same node, so that their gradients ride in its adjoint kernels (SmallifyLoss /
                # VariationalDropoutLoss pick them up through cached_penalties())
                n = len(coeffs)
                if os.environ.get('LFGC_NO_PENALTY_FOLD') or not self._penalty_wanted:   # env: diagnostics (tools/microbench/penalty_fold_ab.py)
                    return ops.DecodeVolumeDropFn.apply(self.filter.filter_rev, self.shape_array, channel_last, thresholds,
                                                        n, *[c.contiguous() for c in coeffs], *factors)
                # NOTE the cache below is handed out ONCE (cached_penalties pops it): a reference to `pen` that outlives
                # the step made the HIP-graph replay of the whole train step 0.25 ms slower (measured; a tensor of the
                # captured region kept alive past the capture), which had hidden the gain of the fold for two layer types
                grid, pen = ops.DecodeVolumePenaltyFn.apply(self.filter.filter_rev, self.shape_array, channel_last,
                                                            thresholds, n, l1_flags,
                                                            *[c.contiguous() for c in coeffs], *factors)
                self._penalty_cache = {'key': self._penalty_key(), 'decode': self._decode_count, 'pen': pen, 'n': n,
                                       'l1_idx': [i for i in range(n) if l1_flags[i] and factors[i] is not None]}
                return grid
            return ops.decode_levels_drop([c.detach() for c in coeffs], [None if f is None else f.detach() for f in factors],
                                          thresholds, self.shape_array, self.filter.filter_rev, channel_last)
        if track:
            return ops.DecodeVolumeFn.apply(self.filter.filter_rev, self.shape_array, channel_last,
                                            *[c.contiguous() for c in coeffs])
        return ops.decode_levels(coeffs, self.shape_array, self.filter.filter_rev, channel_last=channel_last)

    def _decoded_channel_last(self) -> torch.Tensor:
        """decode_volume() in the sampler's layout (G,G,G,Cs).  Differentiable when grads are enabled;
        cached across calls in no-grad mode while no coefficient changed (the reference re-decodes the
        whole grid for every 32^3 tile, visualization/OutputToVTK.py:41)."""
        track = torch.is_grad_enabled() and any(p.requires_grad for p in self.feature_grid)
        cacheable = (not track) and (not self.training) and self._identity_drop()
        key = self._key(list(self.feature_grid) + [self.filter.filter_rev]) if cacheable else None
        if cacheable and self._grid_cache is not None and self._grid_cache[0] == key:
            return self._grid_cache[1]
        grid = self._decode(channel_last=True)
        if cacheable:
            self._grid_cache = (key, grid)
        return grid

    def forward(self, input):
        # the mode is resolved once per forward; the autograd nodes built below keep it in their ctx for the backward
        with ops.deterministic_mode(self.deterministic):
            return self._forward(input)

    def _forward(self, input):
        grid_cl = self._decoded_channel_last()

        orig_shape = input.shape
        if not self.training:
            # reference :57-60 flattens the tile with squeeze()/view (which breaks on size-1 axes and, on
            # torch >= 2, at :78); the intended semantics are implemented: flatten, run, restore, clamp.
            input = input.reshape(-1, orig_shape[-1])
        if input.dim() != 2 or input.shape[-1] != self.d_in:
            raise ValueError('expected positions of shape (N, %d), got %s' % (self.d_in, tuple(orig_shape)))

        weights, biases = self._mlp_params()
        if not torch.is_grad_enabled():
            # grad mode is decided HERE: inside an autograd Function's forward it always reads "off", and the parameters'
            # requires_grad flags say nothing about it -- under no_grad (field_from_net, validation) no stash is written
            # (it is ~2.2 KB per sample) and the eval clamp runs inside the kernel
            y, _ = ops.forward_raw(self._descriptor(), grid_cl.detach(), self._packed(), pos=input.detach(),
                                   clamp=not self.training, want_stash=False, precision=self.precision)
            x = y.view(-1, 1)
            return x if self.training else x.view(*orig_shape[:-1], 1)
        x = ops.SampleDecodeFn.apply(self._descriptor(), input, grid_cl, self._packed(), self.num_layer,
                                     self.precision, *weights, *biases)

        if not self.training:
            x = x.view(*orig_shape[:-1], 1).clamp(-1, 1)
        return x

    def value_and_gradient(self, input, max_stash_bytes: int = 1 << 30):
        """(value, gradient) of the network at ``input``: what the reference gets by marking the positions requires_grad
        (training/training.py:99) and differentiating the output, without an autograd graph.

        ``input`` is (N, 3), or any (..., 3) shape in eval mode, as ``forward`` takes it.  ``value`` is what ``forward``
        returns in the current mode ((N, 1) unclamped in training mode, (..., 1) clamped to [-1, 1] in eval mode).
        ``gradient`` has ``input``'s shape and is the derivative of the UNCLAMPED output with respect to the normalised
        positions, also where the eval value saturates: a renderer wants a normal there, not the clamp's zero.  It jumps
        at the cell faces of the feature grid (trilinear sampling), and its sampler part is zero outside [-1, 1].

        Works in train and eval mode, with or without ``torch.no_grad()``; never touches a parameter's ``.grad``.  Runs in
        chunks of ``ops.gradient_chunk_samples`` samples so that the stash (2 240 bytes per sample for the 32-channel 4 x 128 net)
        stays within ``max_stash_bytes``; one stash buffer serves every chunk.  Honours ``self.precision`` and its range
        fallback; uses the decoded-grid and packed-blob caches under their usual rule (eval mode only)."""
        ops._require_hip(input)
        orig_shape = input.shape
        with torch.no_grad():
            pos = input.detach()
            if not self.training:
                pos = pos.reshape(-1, orig_shape[-1])
            if pos.dim() != 2 or pos.shape[-1] != self.d_in:
                raise ValueError('expected positions of shape (N, %d), got %s' % (self.d_in, tuple(orig_shape)))
            pos = ops._f32c(pos)
            grid_cl, packed, desc = self._decoded_channel_last(), self._packed(), self._descriptor()
            n = pos.shape[0]
            value = torch.empty(n, dtype=torch.float32, device=pos.device)
            grad = torch.empty((n, 3), dtype=torch.float32, device=pos.device)
            chunk = ops.gradient_chunk_samples(desc, n, max_stash_bytes)
            stash = None
            for b in range(0, n, chunk):
                e = min(b + chunk, n)
                _, stash = ops.forward_raw(desc, grid_cl, packed, pos=pos[b:e], clamp=not self.training, want_stash=True,
                                           out=value[b:e], precision=self.precision, stash=stash)
                ops.input_gradient_raw(desc, grid_cl, packed, pos[b:e], stash, precision=self.precision, out=grad[b:e])
        value = value.view(-1, 1) if self.training else value.view(*orig_shape[:-1], 1)
        return value, grad.view(orig_shape)

    # ---- wavelet representation of the grid (reference :83-108) ------------------------------------------
    def encode_volume(self, feature_volume, num_levels=None):
        if num_levels is None:
            num_levels = min(dwt_max_level(s, self.filter.filter_length) for s in feature_volume.shape[-3:])
        features, shapes = [], []
        data = feature_volume.detach().unsqueeze(0)
        for _ in range(num_levels):
            filtered, shape = self.filter.encode(data)
            features.append(filtered[0, :, 1:])
            shapes.append(shape)
            data = filtered[:, :, 0]
        features = [data[0]] + [*reversed(features)]
        shape_array = np.asarray(shapes[::-1], dtype=int)
        return features, shape_array

    def decode_volume(self) -> torch.Tensor:
        """Dense grid (C,G,G,G), channel-first like the reference's decode_volume()."""
        with ops.deterministic_mode(self.deterministic):
            return self._decode(channel_last=False)

    # ---- pruning bookkeeping (reference :110-140): pure tensor logic on the drop layers' own methods ------
    def save_dropvalues_on_grid(self, device):
        if isinstance(self.drop[0], nn.Identity):
            return torch.tensor(0, dtype=torch.float32)
        f_grid = [d.multiply_values_with_dropout(grid, device) for grid, d in zip(self.feature_grid, self.drop)]
        self.feature_grid = nn.ParameterList([nn.Parameter(f, requires_grad=True) for f in f_grid])
        zeros = 0
        for grid in f_grid:
            zeros += (grid.numel() - torch.count_nonzero(grid))
        binary_mask_in_floats = torch.tensor(0, dtype=torch.float32)
        for d in self.drop:
            binary_mask_in_floats += d.size_layer()
        return zeros - binary_mask_in_floats / 32.0

    def remove_drop_layers(self, device):
        binary_masks = []
        for dropl in self.drop:
            if isinstance(dropl, nn.Identity):
                return
            binary_masks.append(dropl.calculate_pruning_mask(device))
        f_grid = [grid * mask for grid, mask in zip(self.feature_grid, binary_masks)]
        self.feature_grid = nn.ParameterList([nn.Parameter(f, requires_grad=True) for f in f_grid])
        self.drop = nn.ModuleList([nn.Identity() for _ in self.drop])
