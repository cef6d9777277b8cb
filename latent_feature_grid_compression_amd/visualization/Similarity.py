"""Structural similarity (SSIM) of volumes and renders on the GPU.

PSNR cannot tell a blurred volume from a noisy one of the same MSE; SSIM compares local means, variances and the
covariance under a sliding window.  Everything here is one HIP entry, ``ops.ssim_plane_sums``: separable windows of 1..16
taps per axis, valid-only (no padding), fp64 moments, one SSIM value per window and their sum per plane of window origins.

    volume_ssim      two resident (X, Y, Z) tensors, walked in x-slabs
    ssim_from_net    the model against the ground truth, the prediction made slab by slab and never resident
    image_ssim       two renders (height * width, C), Wang et al.'s 11-tap Gaussian window per channel

A plane sum has the same bits wherever the slab that holds it was cut, and the slabs' sums are folded left to right in
fp64 on the host, so the mean does not depend on ``max_slab_voxels``.  Two inputs of equal contents give exactly 1.0.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops


def ssim_weights(size: int, gaussian: bool = False, sigma: float = 1.5) -> np.ndarray:
    """fp64 weights of one axis, normalised to sum 1: uniform, or exp(-x^2 / 2 sigma^2) centred on the window."""
    size = int(size)
    if size < 1:
        raise ValueError('a window needs at least one tap, got %d' % size)
    if not gaussian:
        return np.full(size, 1.0 / size, dtype=np.float64)
    sigma = float(sigma)
    if not 0.0 < sigma < float('inf'):
        raise ValueError('sigma must be positive and finite, got %r' % sigma)
    x = np.arange(size, dtype=np.float64) - 0.5 * (size - 1)
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return g / g.sum()


def _triple(v, what: str) -> Tuple[int, int, int]:
    if isinstance(v, (int, np.integer)):
        return (int(v),) * 3
    v = tuple(int(t) for t in v)
    if len(v) != 3:
        raise ValueError('%s must be one int or one per axis, got %s' % (what, v))
    return v


def ssim_slabs(n0: int, plane_voxels: int, window: int, stride: int, max_slab_voxels: int) -> List[Tuple[int, int, int, int]]:
    """(p0, p1, x0, x1) per slab: the origin planes [p0, p1) of axis 0 need the input planes [x0, x1) = [p0 stride,
    (p1 - 1) stride + window).  A slab holds at most ``max_slab_voxels`` voxels but at least one origin plane; consecutive
    slabs overlap by window - stride input planes, and every origin plane belongs to exactly one slab."""
    m0 = (n0 - window) // stride + 1
    planes = int(max_slab_voxels) // max(1, int(plane_voxels))
    per_slab = max(1, (planes - window) // stride + 1)
    return [(p0, min(p0 + per_slab, m0), p0 * stride, (min(p0 + per_slab, m0) - 1) * stride + window)
            for p0 in range(0, m0, per_slab)]


def _constants(data_range: float, lengths, sample_covariance: bool) -> Tuple[float, float, float]:
    L = float(data_range)
    if not 0.0 < L < float('inf'):
        raise ValueError('the data range is %r: SSIM needs a positive, finite range (pass data_range)' % L)
    cov_norm = 1.0
    if sample_covariance:
        NP = lengths[0] * lengths[1] * lengths[2]
        if NP < 2:
            raise ValueError('the sample covariance needs a window of at least two taps')
        cov_norm = NP / (NP - 1.0)
    return (0.01 * L) ** 2, (0.03 * L) ** 2, cov_norm


def _fold(plane_sums: torch.Tensor, windows: int) -> float:
    total = 0.0
    for v in plane_sums.tolist():                 # left to right, fp64, on the host
        total += v
    return total / windows


def _slab_ssim(slab_fn: Callable, shape, lengths, strides, weights, c1, c2, cov_norm, max_slab_voxels, return_map):
    m = ops.ssim_window_counts(shape, lengths, strides)
    sums, maps = [], []
    for _, _, x0, x1 in ssim_slabs(shape[0], shape[1] * shape[2], lengths[0], strides[0], max_slab_voxels):
        xa, xb = slab_fn(x0, x1)
        s, mp = ops.ssim_plane_sums(xa, xb, weights, strides, c1, c2, cov_norm, want_map=return_map)
        sums.append(s)
        maps.append(mp)
    mean = _fold(torch.cat(sums), m[0] * m[1] * m[2])
    return (mean, torch.cat(maps)) if return_map else mean


def volume_ssim(a: torch.Tensor, b: torch.Tensor, window=7, stride=1, gaussian: bool = False, sigma: float = 1.5,
                data_range: Optional[float] = None, sample_covariance: bool = False, max_slab_voxels: int = 1 << 24,
                return_map: bool = False):
    """Mean SSIM of two device tensors (X, Y, Z); with ``return_map`` also the fp64 map (m0, m1, m2) on the device.

    ``window`` / ``stride``: one int or one per axis; uniform weights, or Gaussian ones of ``sigma``.  ``b`` is the ground
    truth: ``data_range=None`` takes max(b) - min(b) over the whole of it, the rule of the project's PSNR (a zero range
    raises ValueError).  ``sample_covariance`` scales the (co)variances by NP / (NP - 1), scikit-image's default; the
    population form is Wang et al.'s.  Windows are valid-only, so the result is the plain mean over
    ((n - w) // s + 1) windows per axis.  The volume is walked in x-slabs of at most ``max_slab_voxels`` voxels and the mean
    is bit-identical for every such limit."""
    if a.shape != b.shape:
        raise ValueError('the two volumes differ in shape: %s and %s' % (tuple(a.shape), tuple(b.shape)))
    lengths, strides = _triple(window, 'window'), _triple(stride, 'stride')
    ops.ssim_window_counts(a.shape, lengths, strides)
    weights = [ssim_weights(w, gaussian, sigma) for w in lengths]
    if data_range is None:
        data_range = float(b.max()) - float(b.min())
    c1, c2, cov_norm = _constants(data_range, lengths, sample_covariance)
    return _slab_ssim(lambda x0, x1: (a[x0:x1], b[x0:x1]), tuple(a.shape), lengths, strides, weights, c1, c2, cov_norm,
                      max_slab_voxels, return_map)


def ssim_from_net(dataset, net, gt_vol: torch.Tensor, window=7, stride=1, gaussian: bool = False, sigma: float = 1.5,
                  data_range: Optional[float] = None, sample_covariance: bool = False, max_slab_voxels: int = 1 << 24,
                  return_map: bool = False, tiled_res: int = 32):
    """``volume_ssim`` of the model's eval-mode reconstruction against ``gt_vol`` (device, the dataset's resolution): each
    slab's prediction comes from ``field_from_net_fused(dataset, net, x0, x1)``, so neither a full prediction nor any
    full-size temporary is ever resident.  Needs eval mode, as ``joint_histogram_from_net`` does."""
    from .OutputToVTK import field_from_net_fused
    if net.training:
        raise ValueError('ssim_from_net compares the eval-mode reconstruction: call net.eval() first')
    res = tuple(int(v) for v in dataset.vol_res_touple)
    if tuple(gt_vol.shape) != res:
        raise ValueError('gt_vol %s does not have the shape of the dataset %s' % (tuple(gt_vol.shape), res))
    lengths, strides = _triple(window, 'window'), _triple(stride, 'stride')
    ops.ssim_window_counts(res, lengths, strides)
    weights = [ssim_weights(w, gaussian, sigma) for w in lengths]
    if data_range is None:
        data_range = float(gt_vol.max()) - float(gt_vol.min())
    c1, c2, cov_norm = _constants(data_range, lengths, sample_covariance)
    ops._require_hip(gt_vol)
    gt = ops._f32c(gt_vol.detach())
    return _slab_ssim(lambda x0, x1: (field_from_net_fused(dataset, net, x0, x1, tiled_res), gt[x0:x1]), res, lengths, strides,
                      weights, c1, c2, cov_norm, max_slab_voxels, return_map)


def image_ssim(a: torch.Tensor, b: torch.Tensor, width: int, height: int, window: int = 11, gaussian: bool = True,
               sigma: float = 1.5, peak: float = 1.0) -> float:
    """Mean SSIM of two renders (height * width, C) as ``render_from_net`` returns them, over all channels: each channel is
    a (height, width) plane with a ``window`` x ``window`` window at stride 1, L = ``peak`` and the population form --
    Wang et al.'s setting with the defaults."""
    if a.shape != b.shape:
        raise ValueError('images differ in shape: %s and %s' % (tuple(a.shape), tuple(b.shape)))
    width, height = int(width), int(height)
    if a.dim() != 2 or a.shape[0] != width * height:
        raise ValueError('an image of %d x %d pixels is (%d, C), got %s' % (width, height, width * height, tuple(a.shape)))
    C = int(a.shape[1])
    lengths, strides = (1, int(window), int(window)), (1, 1, 1)
    m = ops.ssim_window_counts((C, height, width), lengths, strides)
    weights = [ssim_weights(w, gaussian, sigma) for w in lengths]
    c1, c2, cov_norm = _constants(peak, lengths, False)
    planes = [t.detach().reshape(height, width, C).permute(2, 0, 1).contiguous() for t in (a, b)]
    sums, _ = ops.ssim_plane_sums(planes[0], planes[1], weights, strides, c1, c2, cov_norm)
    return _fold(sums, m[0] * m[1] * m[2])
