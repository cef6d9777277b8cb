"""Direct volume rendering of the compressed model: rays, samples, transfer function, front-to-back compositing and
the dropping of finished rays around the fused forward kernel.  The reference has no renderer.

    origins, dirs = pinhole_rays(eye, look_at, up, 40.0, 640, 480, device='cuda')
    image = render_from_net(dataset, net, origins, dirs, TransferFunction(table))        # (R, 4): r, g, b, opacity

Emission / absorption only (no scattering, no shadows), one GPU.  All coordinates are the network's normalised
coordinates: the volume fills the box +-dataset.scales, which is isotropic in voxel units, so one step length serves
all three axes.

The loop marches every live ray ``block_steps`` samples at a time: ops.ray_samples lays the samples of a ray out as
consecutive rows (a 32-sample tile of the forward kernel is 32 consecutive steps of ONE ray, so its gathers share
cells), ``value_fn`` evaluates them, ops.ray_composite folds them into the per-ray state, and ops.ray_compact keeps the
rays that still have steps left and are not yet opaque.  The one 8-byte read-back of that list's length per block of
``block_steps`` steps is the only synchronisation.  There is no CPU form: CPU tensors raise LfgcError.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Sequence, Tuple

import torch

from .. import ops


# ---- rays (pure torch: these also run on the CPU) -----------------------------------------------------------------------

def _vec3(v, device) -> torch.Tensor:
    return torch.as_tensor(v, dtype=torch.float64, device=device).reshape(3)


def _camera_frame(eye, look_at, up, device):
    eye, look_at, up = _vec3(eye, device), _vec3(look_at, device), _vec3(up, device)
    forward = look_at - eye
    if float(forward.norm()) == 0.0:
        raise ValueError('eye and look_at coincide')
    forward = forward / forward.norm()
    right = torch.linalg.cross(forward, up)
    if float(right.norm()) == 0.0:
        raise ValueError('up is parallel to the viewing direction')
    right = right / right.norm()
    return eye, forward, right, torch.linalg.cross(right, forward)


def _pixel_offsets(width: int, height: int, device):
    """Pixel centres as offsets in [-1, 1] (x to the right, y up), row-major over the image: row 0 is the top row."""
    if width < 1 or height < 1:
        raise ValueError('image must have at least one pixel')
    x = (2.0 * (torch.arange(width, dtype=torch.float64, device=device) + 0.5) / width - 1.0).view(1, width)
    y = (1.0 - 2.0 * (torch.arange(height, dtype=torch.float64, device=device) + 0.5) / height).view(height, 1)
    return x.expand(height, width).reshape(-1, 1), y.expand(height, width).reshape(-1, 1)


def pinhole_rays(eye, look_at, up, fov_y_deg: float, width: int, height: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(origins, dirs), each (height*width, 3) fp32, row-major over the image (row 0 = top), unit directions.  The image
    plane spans ``fov_y_deg`` vertically between the top and bottom EDGES of the image; pixels are square; rays pass
    through pixel centres (an odd-sized image has a ray straight through ``look_at``)."""
    if not 0.0 < float(fov_y_deg) < 180.0:
        raise ValueError('fov_y_deg must lie in (0, 180)')
    eye, forward, right, true_up = _camera_frame(eye, look_at, up, device)
    x, y = _pixel_offsets(width, height, device)
    half_h = math.tan(math.radians(float(fov_y_deg)) / 2.0)
    half_w = half_h * width / height
    d = forward.view(1, 3) + x * half_w * right.view(1, 3) + y * half_h * true_up.view(1, 3)
    d = d / d.norm(dim=1, keepdim=True)
    return eye.view(1, 3).expand_as(d).to(torch.float32).contiguous(), d.to(torch.float32).contiguous()


def orthographic_rays(eye, look_at, up, view_height: float, width: int, height: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Parallel rays along look_at - eye from an image plane through ``eye`` that is ``view_height`` tall (normalised
    units, edge to edge) and view_height * width / height wide.  Same shapes and pixel order as ``pinhole_rays``."""
    if not float(view_height) > 0.0:
        raise ValueError('view_height must be positive')
    eye, forward, right, true_up = _camera_frame(eye, look_at, up, device)
    x, y = _pixel_offsets(width, height, device)
    half_h = float(view_height) / 2.0
    half_w = half_h * width / height
    o = eye.view(1, 3) + x * half_w * right.view(1, 3) + y * half_h * true_up.view(1, 3)
    return o.to(torch.float32).contiguous(), forward.view(1, 3).expand_as(o).to(torch.float32).contiguous()


# ---- transfer function --------------------------------------------------------------------------------------------------

class TransferFunction:
    """Piecewise-linear table over the value range [v_min, v_max]: K >= 2 rows of (r, g, b, extinction per unit normalised
    length), the first at v_min and the last at v_max; values outside the range take the end rows."""

    def __init__(self, table, v_min: float = -1.0, v_max: float = 1.0):
        table = torch.as_tensor(table, dtype=torch.float32).detach()
        if table.dim() != 2 or table.shape[1] != 4 or table.shape[0] < 2:
            raise ValueError('transfer function table must be (K, 4) with K >= 2, got %s' % (tuple(table.shape),))
        if not bool(torch.isfinite(table).all()):
            raise ValueError('transfer function table must be finite')
        if bool((table[:, 3] < 0).any()):
            raise ValueError('extinction (column 3) must be >= 0')
        if not float(v_max) > float(v_min):
            raise ValueError('v_max must exceed v_min')
        self.table = table.contiguous()
        self.v_min, self.v_max = float(v_min), float(v_max)
        self._on = {}

    def on(self, device) -> torch.Tensor:
        """The table on ``device`` (cached)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.table.to(device).contiguous()
        return t


# ---- the marching loop --------------------------------------------------------------------------------------------------

def max_steps_for(box_min, box_max, step: float) -> int:
    """Upper limit of steps per ray handed to the clip: twice the box diagonal in steps, at least one block."""
    diag = math.sqrt(sum((float(b) - float(a)) ** 2 for a, b in zip(box_min, box_max)))
    return max(32, int(math.ceil(2.0 * diag / float(step))))


def render(value_fn: Callable, origins: torch.Tensor, dirs: torch.Tensor, tf: TransferFunction, step: float, box_min, box_max,
           block_steps: int = 32, opacity_limit: float = 0.999, shading: Optional[str] = None,
           max_samples_per_launch: int = 1 << 22, ka: float = 0.3, kd: float = 0.7, t_min: float = 0.0,
           t_max: float = float('inf'), stats: Optional[dict] = None) -> torch.Tensor:
    """(R, 4): premultiplied r, g, b and the opacity 1 - T of every ray (``background`` puts it over a colour).

    ``value_fn(pos (n, 3))`` returns the n values, or (values, gradients (n, 3)) when ``shading='headlight'`` (two-sided
    diffuse with the light at the eye: ka + kd |g.d| / |g|).  ``step`` is the sample distance in normalised units; a ray's
    last segment is cut at the box, so the image is continuous in ``step``.  ``opacity_limit``: a ray stops contributing
    once its opacity reaches it.  ``dirs`` are normalised here.

    Loop: clip -> compact the hits -> read the count; while rays are live: for chunks of the live list with
    chunk * block_steps <= max_samples_per_launch: samples -> value_fn -> composite; then compact and read the count.
    That 8-byte read-back per block of ``block_steps`` steps is the only synchronisation; a ray's arithmetic does not
    depend on the chunk or list it sits in, so the image does not depend on ``max_samples_per_launch``.

    ``stats``: a dict that receives 'live' (live rays per block), 'samples' (rows evaluated) and 'blocks'."""
    ops._require_hip(origins, dirs)
    if shading not in (None, 'headlight'):
        raise ValueError("shading must be None or 'headlight'")
    S = int(block_steps)
    if S < 32 or S % 32:
        raise ValueError('block_steps must be a positive multiple of 32')
    if not float(step) > 0.0:
        raise ValueError('step must be positive')
    if not 0.0 < float(opacity_limit) <= 1.0:
        raise ValueError('opacity_limit must lie in (0, 1]')
    origins, dirs = ops._f32c(origins.detach()), ops._f32c(dirs.detach())
    if origins.dim() != 2 or origins.shape[1] != 3 or dirs.shape != origins.shape:
        raise ValueError('origins and dirs must both be (R, 3)')
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    R, dev = origins.shape[0], origins.device
    max_steps = max_steps_for(box_min, box_max, step)
    if max_steps > (1 << 30):
        raise ValueError('step %g is too small for the box: more than 2^30 steps per ray' % step)
    chunk = max(1, int(max_samples_per_launch) // S)
    table = tf.on(dev)
    state = torch.zeros((R, 4), dtype=torch.float32, device=dev)
    state[:, 3] = 1.0
    live_counts, n_samples = [], 0
    if R:
        t_near, t_far, n_steps = ops.ray_clip(origins, dirs, box_min, box_max, step, max_steps, t_min, t_max)
        k_next = torch.zeros(R, dtype=torch.int32, device=dev)
        live = ops.ray_compact(None, n_steps, k_next, state, opacity_limit)
        while live.numel():
            live_counts.append(int(live.numel()))
            for b in range(0, live.numel(), chunk):
                part = live[b:b + chunk]
                pos = ops.ray_samples(part, origins, dirs, t_near, t_far, n_steps, k_next, step, S)
                out = value_fn(pos)
                values, grad = out if shading else (out, None)
                if shading and grad is None:
                    raise ValueError("shading='headlight' needs value_fn to return (values, gradients)")
                ops.ray_composite(part, values, grad, dirs, t_near, t_far, n_steps, k_next, step, S, table, tf.v_min, tf.v_max,
                                  opacity_limit, state, ka, kd)
                n_samples += pos.shape[0]
            live = ops.ray_compact(live, n_steps, k_next, state, opacity_limit)
    if stats is not None:
        stats.update(live=live_counts, samples=n_samples, blocks=len(live_counts))
    state[:, 3] = 1.0 - state[:, 3]
    return state


def background(image: torch.Tensor, colour) -> torch.Tensor:
    """(R, 3): the premultiplied render over a constant background colour, rgb + T * colour with T = 1 - opacity."""
    bg = torch.as_tensor(colour, dtype=image.dtype, device=image.device).reshape(1, 3)
    return image[:, :3] + (1.0 - image[:, 3:4]) * bg


def _scales_of(dataset_or_scales) -> Sequence[float]:
    s = getattr(dataset_or_scales, 'scales', dataset_or_scales)
    s = [float(v) for v in (s.tolist() if hasattr(s, 'tolist') else s)]
    if len(s) != 3 or min(s) <= 0.0:
        raise ValueError('scales must be three positive numbers')
    return s


def render_from_net(dataset_or_scales, net, origins: torch.Tensor, dirs: torch.Tensor, tf: TransferFunction,
                    step: Optional[float] = None, **kwargs) -> torch.Tensor:
    """``render`` of the compressed model: the values are the clamped eval-mode output of ``net`` (ops.forward_raw under
    no_grad; ``net.value_and_gradient`` in eval mode when ``shading='headlight'``), the box is +-scales.  ``step`` defaults
    to half a voxel of the volume, 1 / max_dim in normalised units (an IndexDataset is needed for that).  Honours
    ``net.precision``; the decoded grid and the packed weights come from the eval-mode caches under their usual rule."""
    ops._require_hip(origins, dirs)
    scales = _scales_of(dataset_or_scales)
    if step is None:
        if not hasattr(dataset_or_scales, 'max_dim'):
            raise ValueError('the default step needs a dataset (max_dim); pass step explicitly with bare scales')
        step = 1.0 / float(dataset_or_scales.max_dim)
    precision = getattr(net, 'precision', 'f16x2')
    if kwargs.get('shading'):
        if net.training:
            raise ValueError("shading='headlight' evaluates net.value_and_gradient in eval mode: call net.eval() first")

        def value_fn(pos):
            v, g = net.value_and_gradient(pos)
            return v.view(-1), g
    else:
        with torch.no_grad():
            desc, grid_cl, packed = net._descriptor(), net._decoded_channel_last(), net._packed()

        def value_fn(pos):
            with torch.no_grad():
                return ops.forward_raw(desc, grid_cl, packed, pos=pos, clamp=True, precision=precision)[0]
    return render(value_fn, origins, dirs, tf, step, [-s for s in scales], scales, **kwargs)


def index_positions(dataset, pos: torch.Tensor) -> torch.Tensor:
    """Inverse of IndexDataset.positions_for: normalised positions -> voxel index units, kept inside [min_idx, max_idx] (a
    sample within rounding of a face of the box must not index past the volume)."""
    dev = pos.device
    mn, mx, sc = dataset.min_idx.to(dev).unsqueeze(0), dataset.max_idx.to(dev).unsqueeze(0), dataset.scales.to(dev).unsqueeze(0)
    return torch.minimum(torch.maximum((pos / sc + 1.0) * 0.5 * (mx - mn) + mn, mn), mx)


def render_from_volume(dataset, volume: torch.Tensor, origins: torch.Tensor, dirs: torch.Tensor, tf: TransferFunction,
                       step: Optional[float] = None, **kwargs) -> torch.Tensor:
    """The same loop over the ground truth: samples are mapped back to index units (``index_positions``) and read with the
    trilinear sampler ops.gt_interp.  Same rays, same transfer function, same step as ``render_from_net`` ->
    ``image_psnr`` of the two is the image-space quality of the compression.  Unshaded only."""
    ops._require_hip(origins, dirs, volume)
    if kwargs.get('shading'):
        raise ValueError('render_from_volume has no gradients: shading is not available')
    scales = _scales_of(dataset)
    if step is None:
        step = 1.0 / float(dataset.max_dim)
    volume = ops._f32c(volume.detach())
    mn, mx, res = dataset.min_idx.tolist(), dataset.max_idx.tolist(), dataset.vol_res.tolist()

    def value_fn(pos):
        return ops.gt_interp(index_positions(dataset, pos), volume, mn, mx, res)
    return render(value_fn, origins, dirs, tf, step, [-s for s in scales], scales, **kwargs)


def image_psnr(a: torch.Tensor, b: torch.Tensor, peak: float = 1.0) -> float:
    """PSNR (dB) between two renders of the same rays over all their channels; inf for identical images."""
    if a.shape != b.shape:
        raise ValueError('images differ in shape: %s and %s' % (tuple(a.shape), tuple(b.shape)))
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float('inf') if mse == 0.0 else 10.0 * math.log10(peak * peak / mse)
