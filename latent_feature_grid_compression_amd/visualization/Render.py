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

Empty-space skipping: ``render_from_net(..., skip=BrickRanges.from_net(dataset, net))`` lets every ray jump over the
blocks of ``block_steps`` steps that lie in bricks of the volume where the transfer function is transparent over the
brick's value range (ops.ray_skip after the clip and after each compositing); the model is not evaluated there.

A ``TransferFunction2D`` over value and gradient magnitude goes wherever a ``TransferFunction`` goes in ``render``,
``render_from_net``, ``render_from_volume`` and ``BrickRanges.occupancy`` (ops.ray_composite2d: every sample then needs its
gradient); ``joint_histogram_from_net`` / ``joint_histogram_from_volume`` count the volume over the same two axes.

First-hit isosurfaces use the same loop with ops.ray_iso_scan in the place of the compositing:

    hits = isosurface_from_net(dataset, net, origins, dirs, iso=0.2)                     # IsoHits: hit, t, position, normal, value
    image = background(shade_isosurface(hits, dirs), (0.0, 0.0, 0.0))

``isosurface_from_volume`` is the ground truth's surface and ``surface_deviation`` the distance between the two.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional, Sequence, Tuple

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
        self._integral = None
        self._integral_on = {}

    def on(self, device) -> torch.Tensor:
        """The table on ``device`` (cached)."""
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.table.to(device).contiguous()
        return t

    def integral(self) -> torch.Tensor:
        """The float64 (K, 4) integral table of ``render(..., preintegrated=True)`` on the CPU (cached): row i is the sum
        over the cells c < i of the cell's mean of (tau r, tau g, tau b, tau), tau = the extinction and both tau and the
        colour linear across a cell (include/lfgc.h: lfgc_ray_composite_preint_f32).  Row 0 is zero; the differences of
        column 3 are the trapezoid areas of the extinction in units of one cell."""
        if self._integral is None:
            t = self.table.to(torch.float64)
            t0, d = t[:-1], t[1:] - t[:-1]
            w0, dw = t0[:, 3:4], d[:, 3:4]
            cell = torch.cat([w0 * t0[:, :3] + 0.5 * (w0 * d[:, :3] + dw * t0[:, :3]) + (dw * d[:, :3]) / 3.0, w0 + 0.5 * dw], 1)
            self._integral = torch.cat([torch.zeros((1, 4), dtype=torch.float64), torch.cumsum(cell, 0)], 0).contiguous()
        return self._integral

    def integral_on(self, device) -> torch.Tensor:
        """``integral()`` on ``device`` (cached)."""
        device = torch.device(device)
        t = self._integral_on.get(device)
        if t is None:
            t = self._integral_on[device] = self.integral().to(device).contiguous()
        return t


class TransferFunction2D:
    """Bilinear table over the value range [v_min, v_max] and the gradient magnitude [0, g_max]: (Kv, Kg, 4) entries of
    (r, g, b, extinction per unit normalised length), Kv, Kg >= 2; row i of the value axis sits at
    v_min + i (v_max - v_min) / (Kv - 1), row j of the gradient axis at j g_max / (Kg - 1); what lies outside takes the
    end rows.  The gradient is the one ``net.value_and_gradient`` returns: per unit of normalised position.  Material
    boundaries have a large |gradient|, homogeneous regions a small one: a table that is transparent at small |gradient|
    shows the boundaries alone."""

    def __init__(self, table, v_min: float = -1.0, v_max: float = 1.0, g_max: float = 1.0):
        table = torch.as_tensor(table, dtype=torch.float32).detach()
        if table.dim() != 3 or table.shape[2] != 4 or table.shape[0] < 2 or table.shape[1] < 2:
            raise ValueError('2-D transfer function table must be (Kv, Kg, 4) with Kv, Kg >= 2, got %s' % (tuple(table.shape),))
        if table.shape[0] * table.shape[1] > 1 << 22:
            raise ValueError('2-D transfer function table must not have more than 2^22 entries')
        if not bool(torch.isfinite(table).all()):
            raise ValueError('transfer function table must be finite')
        if bool((table[..., 3] < 0).any()):
            raise ValueError('extinction (column 3) must be >= 0')
        if not float(v_max) > float(v_min):
            raise ValueError('v_max must exceed v_min')
        if not 0.0 < float(g_max) < float('inf'):
            raise ValueError('g_max must be positive and finite')
        self.table = table.contiguous()
        self.v_min, self.v_max, self.g_max = float(v_min), float(v_max), float(g_max)
        self._on = {}
        self._projection = None

    on = TransferFunction.on

    def value_projection(self) -> TransferFunction:
        """The 1-D table over the value alone that is at least as opaque as this one at any gradient: Kv rows, the
        extinction of a row is the largest of its Kg entries (its colour their mean).  Where it is transparent, so is this
        table for every gradient -- what ``BrickRanges.occupancy`` needs.  Cached."""
        if self._projection is None:
            rows = torch.cat([self.table[..., :3].mean(1), self.table[..., 3].amax(1, keepdim=True)], 1)
            self._projection = TransferFunction(rows, self.v_min, self.v_max)
        return self._projection

    @classmethod
    def from_ramp(cls, tf: TransferFunction, g_lo: float, g_hi: float, Kg: int = 64, g_max: Optional[float] = None) -> 'TransferFunction2D':
        """Boundary emphasis: the colours of the 1-D ``tf`` at every gradient, its extinction times a linear ramp in the
        gradient magnitude that is 0 up to ``g_lo`` and 1 from ``g_hi`` on.  ``Kg`` rows over [0, g_max] (default
        g_max = g_hi)."""
        g_lo, g_hi = float(g_lo), float(g_hi)
        g_max = g_hi if g_max is None else float(g_max)
        if not 0.0 <= g_lo < g_hi or g_hi == float('inf'):
            raise ValueError('the ramp needs 0 <= g_lo < g_hi < inf')
        if int(Kg) != Kg or int(Kg) < 2:
            raise ValueError('Kg must be an integer >= 2')
        if not 0.0 < g_max < float('inf'):
            raise ValueError('g_max must be positive and finite')
        g = torch.arange(int(Kg), dtype=torch.float64) * (g_max / (int(Kg) - 1))
        ramp = ((g - g_lo) / (g_hi - g_lo)).clamp(0.0, 1.0)
        table = tf.table.to(torch.float64).unsqueeze(1).repeat(1, int(Kg), 1)
        table[..., 3] *= ramp.view(1, -1)
        return cls(table.to(torch.float32), tf.v_min, tf.v_max, g_max)


# ---- the marching loop --------------------------------------------------------------------------------------------------

def max_steps_for(box_min, box_max, step: float) -> int:
    """Upper limit of steps per ray handed to the clip: twice the box diagonal in steps, at least one block."""
    diag = math.sqrt(sum((float(b) - float(a)) ** 2 for a, b in zip(box_min, box_max)))
    return max(32, int(math.ceil(2.0 * diag / float(step))))


def _march(chunk_step: Callable, origins: torch.Tensor, dirs: torch.Tensor, step: float, box_min, box_max, block_steps: int,
           opacity_limit: float, max_samples_per_launch: int, t_min: float, t_max: float, stats: Optional[dict],
           n_buffers: int = 0, skip: Optional[SimpleNamespace] = None) -> SimpleNamespace:
    """The marching loop of ``render`` and ``isosurface`` (their docstrings describe it) with ``chunk_step(rays, part, pos)``
    in the place of the compositing: it evaluates the ``block_steps`` positions per ray of ``part`` laid out in ``pos`` and
    folds them into ``rays.state`` and ``rays.k_next``.  Returns ``rays``: origins, unit dirs, state (R, 4) and ``n_buffers``
    more zeroed (R, 4) ``buffers``; with R > 0 also t_near, t_far, n_steps, k_next.  ``stats``: 'live', 'samples', 'blocks'.

    ``skip`` (occ, cells, brick: an occupancy table of ``BrickRanges``): ops.ray_skip moves every ray over its empty
    blocks once after the clip and, for the rays of a chunk, after each ``chunk_step`` -- before the compaction that
    follows anyway, so there is no further compaction or read-back.  ``rays.skipped`` counts the jumps per ray and
    ``stats`` also gets 'skipped_blocks'."""
    S = int(block_steps)
    if S < 32 or S % 32:
        raise ValueError('block_steps must be a positive multiple of 32')
    if not float(step) > 0.0:
        raise ValueError('step must be positive')
    ops._require_hip(origins, dirs)
    origins, dirs = ops._f32c(origins.detach()), ops._f32c(dirs.detach())
    if origins.dim() != 2 or origins.shape[1] != 3 or dirs.shape != origins.shape:
        raise ValueError('origins and dirs must both be (R, 3)')
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    R, dev = origins.shape[0], origins.device
    max_steps = max_steps_for(box_min, box_max, step)
    if max_steps > (1 << 30):
        raise ValueError('step %g is too small for the box: more than 2^30 steps per ray' % step)
    chunk = max(1, int(max_samples_per_launch) // S)
    state = torch.zeros((R, 4), dtype=torch.float32, device=dev)
    state[:, 3] = 1.0
    buffers = [torch.zeros((R, 4), dtype=torch.float32, device=dev) for _ in range(n_buffers)]
    rays = SimpleNamespace(origins=origins, dirs=dirs, state=state, buffers=buffers)
    live_counts, n_samples = [], 0
    if R:
        rays.t_near, rays.t_far, rays.n_steps = ops.ray_clip(origins, dirs, box_min, box_max, step, max_steps, t_min, t_max)
        rays.k_next = torch.zeros(R, dtype=torch.int32, device=dev)
        jump = None
        if skip is not None:
            rays.skipped = torch.zeros(R, dtype=torch.int32, device=dev)

            def jump(part):
                ops.ray_skip(part, origins, dirs, rays.t_near, rays.t_far, rays.n_steps, rays.k_next, step, S, box_min, box_max,
                             skip.cells, skip.brick, skip.occ, rays.skipped)
            jump(None)
        live = ops.ray_compact(None, rays.n_steps, rays.k_next, state, opacity_limit)
        while live.numel():
            live_counts.append(int(live.numel()))
            for b in range(0, live.numel(), chunk):
                part = live[b:b + chunk]
                pos = ops.ray_samples(part, origins, dirs, rays.t_near, rays.t_far, rays.n_steps, rays.k_next, step, S)
                chunk_step(rays, part, pos)
                n_samples += pos.shape[0]
                if jump is not None:
                    jump(part)
            live = ops.ray_compact(live, rays.n_steps, rays.k_next, state, opacity_limit)
    if stats is not None:
        stats.update(live=live_counts, samples=n_samples, blocks=len(live_counts))
        if skip is not None:
            stats.update(skipped_blocks=int(rays.skipped.sum()) if R else 0)
    return rays


def render(value_fn: Callable, origins: torch.Tensor, dirs: torch.Tensor, tf: TransferFunction, step: float, box_min, box_max,
           block_steps: int = 32, opacity_limit: float = 0.999, shading: Optional[str] = None,
           max_samples_per_launch: int = 1 << 22, ka: float = 0.3, kd: float = 0.7, t_min: float = 0.0,
           t_max: float = float('inf'), stats: Optional[dict] = None, skip: Optional['BrickRanges'] = None,
           skip_margin: Optional[float] = None, preintegrated: bool = False) -> torch.Tensor:
    """(R, 4): premultiplied r, g, b and the opacity 1 - T of every ray (``background`` puts it over a colour).

    ``skip``: ``BrickRanges`` of the field ``value_fn`` evaluates, over the same box.  A ray then jumps over every block of
    ``block_steps`` steps whose samples all lie in bricks where ``tf`` is transparent on the brick's value range widened by
    ``skip_margin`` (default: ``skip.default_margin``); ``value_fn`` is not called there.  Where every skipped sample has
    an extinction of exactly zero the image is the unskipped image bit for bit; ``stats`` also gets 'skipped_blocks'.

    ``value_fn(pos (n, 3))`` returns the n values, or (values, gradients (n, 3)) when ``shading='headlight'`` (two-sided
    diffuse with the light at the eye: ka + kd |g.d| / |g|).  ``step`` is the sample distance in normalised units; a ray's
    last segment is cut at the box, so the image is continuous in ``step``.  ``opacity_limit``: a ray stops contributing
    once its opacity reaches it.  ``dirs`` are normalised here.

    ``tf`` may be a ``TransferFunction2D`` over value and gradient magnitude.  ``value_fn`` must then return (values,
    gradients) whether or not ``shading`` is set, the gradients per unit of normalised position (the units of ``tf.g_max``);
    ``shading='headlight'`` combines with it and uses the same gradients.

    ``preintegrated=True`` composites with pre-integrated classification (ops.ray_composite_preint): a sample stands for
    the slab between itself and the sample before it, under the mean of ``tf`` over the value range the slab spans
    (``tf.integral()``), not for its segment under ``tf`` at its own value.  Where the field is linear between samples
    the opacity does not depend on ``step``, so thin features of ``tf`` survive a large step; self-attenuation inside a
    slab is not modelled.  The samples, and with them the calls of ``value_fn``, are the same.  1-D tables only: a
    ``TransferFunction2D`` raises ValueError.  With ``skip`` the occupancy table is the same (a brick is empty iff ``tf``
    is transparent over its widened range, which is also what a slab inside it integrates to), but the image is NOT
    promised to equal the unskipped one bit for bit: the slab that straddles a jump is replaced by an opening half slab
    behind it and the last sample before the jump gets no trailing half, so a ray may differ by its number of jumps times
    1 - exp(-tau_max * step).  The default, False, changes nothing.

    Loop: clip -> compact the hits -> read the count; while rays are live: for chunks of the live list with
    chunk * block_steps <= max_samples_per_launch: samples -> value_fn -> composite; then compact and read the count.
    That 8-byte read-back per block of ``block_steps`` steps is the only synchronisation; a ray's arithmetic does not
    depend on the chunk or list it sits in, so the image does not depend on ``max_samples_per_launch``.

    ``stats``: a dict that receives 'live' (live rays per block), 'samples' (rows evaluated) and 'blocks'."""
    if preintegrated and isinstance(tf, TransferFunction2D):
        raise ValueError('preintegrated=True needs a 1-D TransferFunction: pre-integration over two axes is not available')
    ops._require_hip(origins, dirs)
    if shading not in (None, 'headlight'):
        raise ValueError("shading must be None or 'headlight'")
    if not 0.0 < float(opacity_limit) <= 1.0:
        raise ValueError('opacity_limit must lie in (0, 1]')
    S, table = int(block_steps), tf.on(origins.device)
    two_d = isinstance(tf, TransferFunction2D)
    pre = tf.integral_on(origins.device) if preintegrated else None

    def composite(rays, part, pos):
        out = value_fn(pos)
        if two_d:
            if not isinstance(out, (tuple, list)) or len(out) != 2 or out[1] is None:
                raise ValueError('a 2-D transfer function needs value_fn to return (values, gradients), with or without shading')
            ops.ray_composite2d(part, out[0], out[1], rays.dirs, rays.t_near, rays.t_far, rays.n_steps, rays.k_next, step, S,
                                table, tf.v_min, tf.v_max, tf.g_max, opacity_limit, rays.state, bool(shading), ka, kd)
            return
        values, grad = out if shading else (out, None)
        if shading and grad is None:
            raise ValueError("shading='headlight' needs value_fn to return (values, gradients)")
        if preintegrated:
            if not hasattr(rays, 'carry_v'):                     # a ray's last value and its step, beside the state
                rays.carry_v = torch.zeros(rays.state.shape[0], dtype=torch.float32, device=rays.state.device)
                rays.carry_k = torch.full((rays.state.shape[0],), -1, dtype=torch.int32, device=rays.state.device)
            ops.ray_composite_preint(part, values, grad, rays.dirs, rays.t_near, rays.t_far, rays.n_steps, rays.k_next, step, S,
                                     table, pre, tf.v_min, tf.v_max, opacity_limit, rays.state, rays.carry_v, rays.carry_k, ka, kd)
            return
        ops.ray_composite(part, values, grad, rays.dirs, rays.t_near, rays.t_far, rays.n_steps, rays.k_next, step, S, table,
                          tf.v_min, tf.v_max, opacity_limit, rays.state, ka, kd)
    table_of = None
    if skip is not None:
        skip.check_box(box_min, box_max)
        table_of = SimpleNamespace(occ=skip.occupancy(tf, skip_margin, origins.device), cells=skip.cells, brick=skip.brick)
    state = _march(composite, origins, dirs, step, box_min, box_max, block_steps, opacity_limit, max_samples_per_launch, t_min,
                   t_max, stats, skip=table_of).state
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
    ``net.precision``; the decoded grid and the packed weights come from the eval-mode caches under their usual rule.

    ``skip=BrickRanges.from_net(dataset, net)`` (``render``) skips the blocks that lie in bricks ``tf`` is transparent
    in, gradient evaluations included; ``skip_margin`` defaults to NET_SKIP_MARGIN.  Ranges taken before the model's
    parameters were last updated raise ValueError.

    A ``TransferFunction2D`` evaluates ``net.value_and_gradient`` for every sample, shaded or not, under the same
    eval-mode rule.

    ``preintegrated=True`` (``render``) composites slabs between consecutive samples under the integral of a 1-D ``tf``:
    the same evaluations of the model, an opacity that does not depend on ``step`` where the model is linear between
    samples.  With ``skip`` the image may differ from the unskipped one at the jumps (``render``)."""
    ops._require_hip(origins, dirs)
    scales = _scales_of(dataset_or_scales)
    step = _default_step(dataset_or_scales, step)
    if kwargs.get('skip') is not None:
        kwargs['skip'].check_fresh(net)
    shading = bool(kwargs.get('shading'))
    if shading and net.training:
        raise ValueError("shading='headlight' evaluates net.value_and_gradient in eval mode: call net.eval() first")
    gradient = shading or isinstance(tf, TransferFunction2D)
    if gradient and net.training:
        raise ValueError('a 2-D transfer function evaluates net.value_and_gradient in eval mode: call net.eval() first')
    net_fn = _net_value_fn(net, values=not gradient)
    return render(lambda pos: net_fn(pos, gradient=gradient), origins, dirs, tf, step, [-s for s in scales], scales, **kwargs)


def _default_step(dataset_or_scales, step):
    """``step``, or half a voxel of the dataset's volume where it is None."""
    if step is None:
        if not hasattr(dataset_or_scales, 'max_dim'):
            raise ValueError('the default step needs a dataset (max_dim); pass step explicitly with bare scales')
        step = 1.0 / float(dataset_or_scales.max_dim)
    return step


def _net_value_fn(net, values: bool = True) -> Callable:
    """``value_fn(pos, gradient=False)`` of the compressed model for ``render``, ``isosurface`` and Mesh.isosurface_mesh:
    the clamped eval-mode output of ``net`` (ops.forward_raw under no_grad), and with ``gradient=True`` (values, gradients)
    of ``net.value_and_gradient``.  Honours ``net.precision``; the decoded grid and the packed weights come from the
    eval-mode caches under their usual rule, here and now -- unless ``values=False`` says that only gradient calls follow."""
    precision = getattr(net, 'precision', 'f16x2')
    if values:
        with torch.no_grad():
            desc, grid_cl, packed = net._descriptor(), net._decoded_channel_last(), net._packed()

    def value_fn(pos, gradient=False):
        if gradient:
            v, g = net.value_and_gradient(pos)
            return v.view(-1), g
        with torch.no_grad():
            return ops.forward_raw(desc, grid_cl, packed, pos=pos, clamp=True, precision=precision)[0]
    return value_fn


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
    ``image_psnr`` of the two is the image-space quality of the compression.  Unshaded only.
    ``skip=BrickRanges.from_volume(dataset, volume)`` skips empty space; the image stays the same bit for bit.
    A ``TransferFunction2D`` takes its gradients from ``volume_value_fn(dataset, volume)(pos, gradient=True)``: central
    differences of the sampler at +- half a voxel, six more samples per sample.
    ``preintegrated=True`` (``render``) composites slabs between consecutive samples under the integral of a 1-D ``tf``;
    with ``skip`` the image is then no longer the unskipped one bit for bit, only within the bound ``render`` states."""
    ops._require_hip(origins, dirs, volume)
    if kwargs.get('shading'):
        raise ValueError('render_from_volume has no gradients: shading is not available')
    scales = _scales_of(dataset)
    step = _default_step(dataset, step)
    value_fn = volume_value_fn(dataset, volume)
    if isinstance(tf, TransferFunction2D):
        value_fn = functools.partial(value_fn, gradient=True)
    return render(value_fn, origins, dirs, tf, step, [-s for s in scales], scales, **kwargs)


# ---- empty-space skipping: value ranges of bricks of the field -------------------------------------------------------------

VOLUME_SKIP_MARGIN = 1e-5     # the three nested fp32 lerps of ops.gt_interp leave their corners' range by < 1e-6 for |v| <= 1
# Twice the larger brick_range_excess of two cfg-3 models at supersample=1, B=8, rounded up to one digit:
# 1.6e-3 with random weights, 0.13 after 113 train steps on the smooth volume.  A guard against an unmeasured model, wide
# enough to leave little to skip; measure brick_range_excess for the model at hand and pass skip_margin to do better.
NET_SKIP_MARGIN = 0.3
_SKIP_GUARD = 0.0625          # LFGC_RAY_SKIP_GUARD of include/lfgc.h (tests/test_render_skip_host.py compares the two)


class BrickRanges:
    """(min, max) of a field over bricks of ``brick``^3 lattice cells, for ``render(..., skip=ranges)``.

    ``minmax`` (nbx, nby, nbz, 2) on the device; ``cells`` lattice cells per axis of the lattice the ranges were taken on
    (``supersample`` times the volume's), ``brick`` the brick edge in those cells; the box is +-``scales``.  The ranges
    bound the field at the lattice points.  Between them a trilinear field stays inside the range of its cell's corners
    up to rounding -- skipping the ground truth is exact --, the network does so only as far as it is smooth at the
    lattice's scale: ``brick_range_excess`` measures that, and ``default_margin`` widens every range by it."""

    def __init__(self, minmax: torch.Tensor, cells, brick: int, scales, default_margin: float, versions=None):
        self.minmax, self.cells, self.brick = minmax, tuple(int(c) for c in cells), int(brick)
        self.scales = [float(s) for s in scales]
        self.default_margin = float(default_margin)
        self.versions = versions
        self._occ = {}

    @classmethod
    def from_volume(cls, dataset, volume: torch.Tensor, brick: int = 8) -> 'BrickRanges':
        """Ranges of the ground truth ``render_from_volume`` samples: exact bounds of the trilinear sampler up to rounding."""
        ops._require_hip(volume)
        volume = ops._f32c(volume.detach())
        res = dataset.vol_res_touple
        if tuple(volume.shape) != tuple(res):
            raise ValueError('volume %s does not have the shape of the dataset %s' % (tuple(volume.shape), tuple(res)))
        minmax = ops.brick_minmax(volume, res, 0, res[0], brick, ops.brick_table(res, brick, volume.device))
        return cls(minmax, [r - 1 for r in res], brick, _scales_of(dataset), VOLUME_SKIP_MARGIN)

    @classmethod
    def from_net(cls, dataset, net, brick: int = 8, supersample: int = 1, max_slab_voxels: int = 1 << 24,
                 timings: Optional[dict] = None) -> 'BrickRanges':
        """Ranges of the compressed model at the points of the volume's lattice: the clamped eval-mode values the renderer
        composites (OutputToVTK.field_from_net_fused), folded x-slab by x-slab of at most ``max_slab_voxels`` values, so
        the volume is never resident.  ``supersample=n`` takes them on an n times finer lattice over the same box (brick
        edge n * ``brick`` fine cells: the same bricks).  Remembers the parameters' versions: ``render_from_net`` refuses
        ranges of a model that has been updated since.  ``timings`` receives 'forward_ms' and 'reduce_ms' (device time)."""
        from ..data.IndexDataset import IndexDataset
        from .OutputToVTK import field_from_net_fused
        n = int(supersample)
        if n < 1 or n != supersample:
            raise ValueError('supersample must be a positive integer')
        cells = [int(r) - 1 for r in dataset.vol_res_touple]
        fine = dataset if n == 1 else IndexDataset(tuple(n * c + 1 for c in cells), build_index_table=False)
        res, edge = fine.vol_res_touple, n * int(brick)
        dev = next(net.parameters()).device
        versions = [p._version for p in net.parameters()]
        minmax = ops.brick_table(res, edge, dev)
        planes = max(1, int(max_slab_voxels) // (res[1] * res[2]))
        spans = []
        for xb in range(0, res[0], planes):
            xe = min(xb + planes, res[0])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timings is not None else None
            if ev:
                ev[0].record()
            values = field_from_net_fused(fine, net, xb, xe)
            if ev:
                ev[1].record()
            ops.brick_minmax(values, res, xb, xe, edge, minmax)
            if ev:
                ev[2].record()
                spans.append(ev)
        if timings is not None:
            torch.cuda.synchronize(dev)
            timings.update(forward_ms=float(sum(e[0].elapsed_time(e[1]) for e in spans)),
                           reduce_ms=float(sum(e[1].elapsed_time(e[2]) for e in spans)), slabs=len(spans))
        return cls(minmax, [n * c for c in cells], edge, _scales_of(dataset), NET_SKIP_MARGIN, versions)

    def occupancy(self, tf: TransferFunction, margin: Optional[float] = None, device=None) -> torch.Tensor:
        """uint8 (nbx, nby, nbz) on the device: 0 where ``tf`` is transparent over the brick's range widened by ``margin``
        (default ``default_margin``), else 1 (ops.brick_occupancy).  Cached per (tf, margin).

        A ``TransferFunction2D`` is tested through its ``value_projection()``: a brick is empty iff every entry that any
        value in its widened range and ANY gradient can interpolate between has extinction 0.  The 2-D lookup then
        yields an extinction of exactly 0 (0 + f (0 - 0) twice, then 0 + h (0 - 0)), so alpha is exactly 0 and the skipped
        image equals the unskipped one bit for bit.  The test is conservative in the gradient axis: the bricks bound the
        value only, so a table that is transparent for small gradients alone skips nothing."""
        margin = self.default_margin if margin is None else float(margin)
        if device is not None and torch.device(device).type == 'cuda' and self.minmax.device != _with_index(device):
            raise ValueError('the ranges live on %s, the rays on %s' % (self.minmax.device, device))
        occ = self._occ.get((tf, margin))
        if occ is None:
            tf1 = tf.value_projection() if isinstance(tf, TransferFunction2D) else tf
            occ = self._occ[(tf, margin)] = ops.brick_occupancy(self.minmax, tf1.on(self.minmax.device), tf1.v_min, tf1.v_max, margin)
        return occ

    def check_box(self, box_min, box_max) -> None:
        f32 = lambda v: torch.tensor([float(x) for x in v], dtype=torch.float32)          # noqa: E731
        if not (torch.equal(f32(box_min), -f32(self.scales)) and torch.equal(f32(box_max), f32(self.scales))):
            raise ValueError('the ranges cover the box +-%s, the render %s .. %s' % (self.scales, list(box_min), list(box_max)))

    def check_fresh(self, net) -> None:
        if self.versions is not None and [p._version for p in net.parameters()] != self.versions:
            raise ValueError('the brick ranges are stale: the parameters of the model have been updated since '
                             'BrickRanges.from_net; a stale table silently drops structure -- build the ranges again')

    def touched_bricks(self, pos: torch.Tensor) -> torch.Tensor:
        """(n, 8) int64: the flat indices into the (nbx, nby, nbz) tables of the bricks the positions (n, 3) touch -- the
        torch form of lfgc_ray_skip_f32's lookup, fp32 operation for operation (entries repeat where the guarded cell
        coordinates fall into one brick)."""
        pos = pos.to(torch.float32)
        lo = -torch.tensor(self.scales, dtype=torch.float32, device=pos.device)
        ext = torch.tensor(self.scales, dtype=torch.float32, device=pos.device) - lo
        cells = torch.tensor(self.cells, dtype=torch.float32, device=pos.device)
        q = (pos - lo) / ext * cells
        top = cells - 1.0
        zero = torch.zeros_like(top)
        pair = [torch.div(torch.minimum(torch.maximum(torch.floor(q + g), zero), top).long(), self.brick, rounding_mode='floor')
                for g in (-_SKIP_GUARD, _SKIP_GUARD)]
        _, nby, nbz = ops.brick_counts(self.cells, self.brick)
        return torch.stack([(pair[i][:, 0] * nby + pair[j][:, 1]) * nbz + pair[k][:, 2]
                            for i in (0, 1) for j in (0, 1) for k in (0, 1)], 1)


def _with_index(device) -> torch.device:
    device = torch.device(device)
    return torch.device('cuda', torch.cuda.current_device()) if device.type == 'cuda' and device.index is None else device


def brick_range_excess(ranges: BrickRanges, value_fn: Callable, n: int = 1 << 20, seed: int = 0) -> float:
    """The largest amount by which ``value_fn`` at ``n`` uniform random positions of the box leaves the range of EVERY
    brick the position touches (0 when each value lies in the range of one of them): what the ranges, taken at lattice
    points, miss of the field between them.  A ``skip_margin`` above it makes skipping exact at these positions."""
    dev = ranges.minmax.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    hi = torch.tensor(ranges.scales, dtype=torch.float32, device=dev)
    flat = ranges.minmax.view(-1, 2)
    worst = 0.0
    for b in range(0, int(n), 1 << 20):
        m = min(1 << 20, int(n) - b)
        pos = ((2.0 * torch.rand((m, 3), generator=gen, device=dev) - 1.0) * hi).contiguous()
        v = value_fn(pos).reshape(-1, 1).to(torch.float32)
        mm = flat[ranges.touched_bricks(pos)]                                   # (m, 8, 2)
        out = torch.maximum(mm[..., 0] - v, v - mm[..., 1]).clamp_min(0.0).amin(1)
        worst = max(worst, float(out.max()))
    return worst


def image_psnr(a: torch.Tensor, b: torch.Tensor, peak: float = 1.0) -> float:
    """PSNR (dB) between two renders of the same rays over all their channels; inf for identical images."""
    if a.shape != b.shape:
        raise ValueError('images differ in shape: %s and %s' % (tuple(a.shape), tuple(b.shape)))
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float('inf') if mse == 0.0 else 10.0 * math.log10(peak * peak / mse)


from .Similarity import image_ssim  # noqa: E402,F401 -- the structural measure of the same pair


# ---- joint histograms of value and gradient magnitude: what a 2-D transfer function is designed on -------------------------

def _joint_histogram(chunks: Callable, bins, v_range, g_max: Optional[float], device) -> Tuple[torch.Tensor, float]:
    """``chunks()`` yields (values (n,), gradients (n, 3)) over the lattice; one pass for g_max where it is None, one to bin."""
    v_min, v_max = (float(v) for v in v_range)
    if g_max is None:
        top = torch.zeros((), dtype=torch.float32, device=device)
        for _, g in chunks():
            top = torch.maximum(top, g.norm(dim=1).max())
        g_max = float(top)
        if not 0.0 < g_max < float('inf'):
            raise ValueError('the largest gradient magnitude is %r: pass g_max' % g_max)
    counts = torch.zeros(tuple(int(b) for b in bins), dtype=torch.int64, device=device)
    for v, g in chunks():
        ops.joint_histogram(v, g, bins, v_min, v_max, g_max, counts)
    return counts, float(g_max)


def joint_histogram_from_net(dataset, net, bins=(64, 64), v_range=(-1.0, 1.0), g_max: Optional[float] = None,
                             max_stash_bytes: int = 1 << 30) -> Tuple[torch.Tensor, float]:
    """(counts int64 (Bv, Bg) on the device, g_max): how many points of the volume lattice have their value in bin i of
    ``v_range`` and their gradient magnitude in bin j of [0, g_max] -- the bins are the cells of a ``TransferFunction2D`` of
    (Bv + 1, Bg + 1) rows over the same ranges, as the renderer finds them (ops.joint_histogram).  The pair is what
    ``net.value_and_gradient`` returns in eval mode at the positions of ops.lattice_slab_positions: the clamped value and
    the gradient of the unclamped output per unit of normalised position.  Covers the lattice in the row chunks of
    ``gradient_field_from_net``, so neither field is ever resident, and the counts do not depend on ``max_stash_bytes``.
    ``g_max=None`` takes the largest magnitude in a first pass over the volume."""
    from .OutputToVTK import _row_chunks
    if net.training:
        raise ValueError('the histogram bins net.value_and_gradient in eval mode: call net.eval() first')
    res = dataset.vol_res_touple
    dev = next(net.parameters()).device
    scales = dataset.scales.tolist()

    def chunks():
        for b, e in _row_chunks(net, res[0], res[1] * res[2], max_stash_bytes):
            v, g = net.value_and_gradient(ops.lattice_slab_positions(res, b, e, 32, scales, dev), max_stash_bytes)
            yield v.view(-1), g
    return _joint_histogram(chunks, bins, v_range, g_max, dev)


def joint_histogram_from_volume(dataset, volume: torch.Tensor, bins=(64, 64), v_range=(-1.0, 1.0), g_max: Optional[float] = None,
                                max_slab_voxels: int = 1 << 22) -> Tuple[torch.Tensor, float]:
    """The same of the ground truth: the volume's own values and OutputToVTK.gradient_ground_truth (central differences of
    the trilinear sampler, per unit of normalised position), x-slabs of at most ``max_slab_voxels`` points at a time."""
    from .OutputToVTK import gradient_ground_truth
    ops._require_hip(volume)
    volume = ops._f32c(volume.detach())
    res = dataset.vol_res_touple
    if tuple(volume.shape) != tuple(res):
        raise ValueError('volume %s does not have the shape of the dataset %s' % (tuple(volume.shape), tuple(res)))
    planes = max(1, int(max_slab_voxels) // (res[1] * res[2]))

    def chunks():
        for b in range(0, res[0], planes):
            e = min(b + planes, res[0])
            yield volume[b:e].reshape(-1), gradient_ground_truth(dataset, volume, b, e)
    return _joint_histogram(chunks, bins, v_range, g_max, volume.device)


# ---- first-hit isosurface ray casting -------------------------------------------------------------------------------------

def _iso_args(iso, refine_steps) -> Tuple[float, int]:
    iso = ops._iso_value(iso)
    n_refine = int(refine_steps)
    if n_refine != refine_steps or not 0 <= n_refine <= 64:
        raise ValueError('refine_steps must be an integer in [0, 64]')
    return iso, n_refine


def _values_and_gradients(out, who: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(values (n,), gradients (n, 3)) fp32 of what ``who``(pos, gradient=True) returned."""
    if not isinstance(out, (tuple, list)) or len(out) != 2 or out[1] is None:
        raise ValueError('normals=True needs %s(pos, gradient=True) to return (values, gradients)' % who)
    return out[0].reshape(-1).to(torch.float32), out[1].reshape(-1, 3).to(torch.float32)


def _unit(g: torch.Tensor) -> torch.Tensor:                       # g / |g| per row, zero where the gradient is zero
    gn = g.norm(dim=1, keepdim=True)
    return torch.where(gn > 0, g / gn, torch.zeros_like(g))


class IsoHits(NamedTuple):
    """Result of ``isosurface``, one row per ray."""
    hit: torch.Tensor          # (R,) bool
    t: torch.Tensor            # (R,) depth along the unit direction; inf for a miss
    position: torch.Tensor     # (R, 3) hit point; 0 for a miss
    normal: torch.Tensor       # (R, 3) unit normal facing the viewer (n . d <= 0); 0 for a miss, a zero gradient or normals=False
    value: torch.Tensor        # (R,) the value value_fn returns at the hit point; 0 for a miss
    t_lo: torch.Tensor         # (R,) the final bracket, t_lo <= t <= t_hi: value - iso changes sign between its ends; inf for a miss
    t_hi: torch.Tensor


def isosurface(value_fn: Callable, origins: torch.Tensor, dirs: torch.Tensor, iso: float, step: float, box_min, box_max,
               block_steps: int = 32, refine_steps: int = 8, normals: bool = True, max_samples_per_launch: int = 1 << 22,
               t_min: float = 0.0, t_max: float = float('inf'), stats: Optional[dict] = None) -> IsoHits:
    """The first point of every ray on the surface value == iso inside the box: an ``IsoHits`` tuple.

    ``value_fn(pos (n, 3))`` returns the n values; with ``normals=True`` it is called once more, at the hit points only,
    as ``value_fn(pos, gradient=True)`` and must then return (values, gradients (n, 3)).  The normal is +-g / |g| with
    the sign that faces the viewer.  ``dirs`` are normalised here.

    A ray is sampled at the midpoints of its ``step``-long segments, as ``render`` samples it.  The first pair of
    neighbouring samples on different sides of ``iso`` (either direction: entering or leaving the set value >= iso
    both hit) brackets the surface; ``refine_steps`` bisections, each one evaluation per bracketed ray, shrink the
    bracket to step * 2^-refine_steps, and one secant step inside it gives ``t``.  A surface the ray crosses twice
    between two neighbouring samples is not seen.  There are NO CAPS: a ray that is already inside the set where it
    enters the box reports the point where it leaves the set, not the box face.

    Loop: clip -> compact the hits -> read the count; while rays march: for chunks of the list with
    chunk * block_steps <= max_samples_per_launch: samples -> value_fn -> scan; then compact (drops the bracketed rays and
    those without steps left) and read the count.  Then over the bracketed rays: refine -> value_fn, ``refine_steps``
    times, and finish.  Every kernel treats a ray by itself, so with a ``value_fn`` that does so too a ray's result does
    not depend on the list or chunk it sits in.

    ``stats``: a dict that receives 'live' (marching rays per block), 'samples' (rows evaluated in the march), 'blocks',
    'bracketed' (rays with a hit) and 'refine_samples' (rows evaluated for the bisection and at the hit points)."""
    iso, n_refine = _iso_args(iso, refine_steps)
    S = int(block_steps)

    def scan(rays, part, pos):
        ops.ray_iso_scan(part, value_fn(pos), rays.t_near, rays.t_far, rays.n_steps, rays.k_next, step, S, iso, rays.state,
                         rays.buffers[0])
    rays = _march(scan, origins, dirs, step, box_min, box_max, block_steps, 1.0, max_samples_per_launch, t_min, t_max, stats,
                  n_buffers=1)
    origins, dirs, state, bracket = rays.origins, rays.dirs, rays.state, rays.buffers[0]
    R, dev = origins.shape[0], origins.device
    hit = state[:, 3] == 0.0
    found = torch.nonzero(hit).view(-1).to(torch.int32)
    t = torch.full((R,), float('inf'), dtype=torch.float32, device=dev)
    position = torch.zeros((R, 3), dtype=torch.float32, device=dev)
    normal = torch.zeros((R, 3), dtype=torch.float32, device=dev)
    value = torch.zeros(R, dtype=torch.float32, device=dev)
    per_launch = max(1, int(max_samples_per_launch))
    n_refined = 0
    for b in range(0, found.numel(), per_launch):
        part = found[b:b + per_launch]
        idx = part.long()
        t_hit, p_hit = _refine_and_finish(value_fn, part, origins, dirs, iso, bracket, n_refine)
        n_refined += (n_refine + 1) * part.numel()
        t[idx], position[idx] = t_hit, p_hit
        if normals:
            value[idx], g = _values_and_gradients(value_fn(p_hit, gradient=True), 'value_fn')
            unit = _unit(g)
            away = (unit * dirs[idx]).sum(1, keepdim=True) > 0
            normal[idx] = torch.where(away, -unit, unit)
        else:
            value[idx] = value_fn(p_hit).reshape(-1).to(torch.float32)
    inf = torch.full_like(t, float('inf'))
    if stats is not None:
        stats.update(bracketed=int(found.numel()), refine_samples=n_refined)
    return IsoHits(hit, t, position, normal, value, torch.where(hit, bracket[:, 0], inf), torch.where(hit, bracket[:, 1], inf))


def _refine_and_finish(value_fn: Callable, rows: torch.Tensor, origins: torch.Tensor, dirs: torch.Tensor, iso: float,
                       bracket: torch.Tensor, n_refine: int):
    """(t, position) of the brackets of ``rows``: ``n_refine`` bisections, each one ``value_fn`` call with one trial point
    per row, then the secant step inside what is left (ops.ray_iso_refine, ops.ray_iso_finish).  ``bracket`` in place."""
    values = None
    for _ in range(n_refine):
        values = value_fn(ops.ray_iso_refine(rows, values, origins, dirs, iso, bracket))
    if values is not None:
        ops.ray_iso_refine(rows, values, origins, dirs, iso, bracket)           # folds the last values in
    return ops.ray_iso_finish(rows, origins, dirs, bracket)


def isosurface_from_net(dataset_or_scales, net, origins: torch.Tensor, dirs: torch.Tensor, iso: float,
                        step: Optional[float] = None, **kwargs) -> IsoHits:
    """``isosurface`` of the compressed model: the values are the clamped eval-mode output of ``net`` (ops.forward_raw under
    no_grad, exactly as ``render_from_net`` evaluates it), the normals come from ``net.value_and_gradient`` in eval mode
    at the hit points only, the box is +-scales, ``step`` defaults to half a voxel.  The output is clamped to [-1, 1], so
    ``iso`` must lie strictly inside that range.  Honours ``net.precision``; the bisection evaluates one sample per
    bracketed ray, so a forward tile then holds samples of 32 different rays."""
    if not -1.0 < float(iso) < 1.0:
        raise ValueError('iso must lie inside the clamp range (-1, 1) of the eval-mode output, got %r' % (iso,))
    ops._require_hip(origins, dirs)
    scales = _scales_of(dataset_or_scales)
    step = _default_step(dataset_or_scales, step)
    if kwargs.get('normals', True) and net.training:
        raise ValueError('normals come from net.value_and_gradient in eval mode: call net.eval() first')
    return isosurface(_net_value_fn(net), origins, dirs, iso, step, [-s for s in scales], scales, **kwargs)


def isosurface_from_volume(dataset, volume: torch.Tensor, origins: torch.Tensor, dirs: torch.Tensor, iso: float,
                           step: Optional[float] = None, **kwargs) -> IsoHits:
    """The same loop over the ground truth: samples are mapped back to index units (``index_positions``) and read with the
    trilinear sampler ops.gt_interp.  Normals are central differences of that sampler at +- half a voxel along each axis
    (six more samples per hit, once per frame, plain torch; one-sided where half a voxel would leave the volume).  Same rays, same iso, same step as ``isosurface_from_net``
    -> ``surface_deviation`` of the two is the surface-space quality of the compression."""
    ops._require_hip(origins, dirs, volume)
    scales = _scales_of(dataset)
    step = _default_step(dataset, step)
    value_fn = volume_value_fn(dataset, volume)
    return isosurface(value_fn, origins, dirs, iso, step, [-s for s in scales], scales, **kwargs)


def volume_value_fn(dataset, volume: torch.Tensor, sampler: Optional[Callable] = None) -> Callable:
    """``value_fn(pos, gradient=False)`` of the ground truth for ``isosurface`` and Mesh.isosurface_mesh: the trilinear
    sampler at normalised positions, and with ``gradient=True`` (values, central differences at +- half a voxel).
    ``sampler(index positions (n, 3), volume)`` replaces ops.gt_interp (Mesh.mesh_value_residual on host tensors)."""
    volume = ops._f32c(volume.detach())
    mn, mx, res = dataset.min_idx.tolist(), dataset.max_idx.tolist(), dataset.vol_res.tolist()

    def sample(pos):
        if sampler is not None:
            return sampler(index_positions(dataset, pos), volume).reshape(-1)
        return ops.gt_interp(index_positions(dataset, pos), volume, mn, mx, res).reshape(-1)

    def value_fn(pos, gradient=False):
        v = sample(pos)
        if not gradient:
            return v
        # half a voxel in normalised units, per axis: index = (pos / scale + 1) / 2 * (max_idx - min_idx) + min_idx.  The two
        # ends are kept inside the box, so the difference is one-sided, over the distance that is left, at a face.
        sc = dataset.scales.to(pos.device, torch.float32)
        h = sc / (dataset.max_idx - dataset.min_idx).clamp(min=1).to(pos.device, torch.float32)
        g = torch.empty_like(pos)
        for a in range(3):
            e = torch.zeros(3, dtype=torch.float32, device=pos.device)
            e[a] = h[a]
            hi, lo = torch.minimum(pos + e, sc), torch.maximum(pos - e, -sc)
            g[:, a] = (sample(hi) - sample(lo)) / (hi[:, a] - lo[:, a])
        return v, g
    return value_fn


def shade_isosurface(hits: IsoHits, dirs: torch.Tensor, colour=(1.0, 1.0, 1.0), ka: float = 0.3, kd: float = 0.7, ks: float = 0.0,
                     shininess: float = 32.0) -> torch.Tensor:
    """(R, 4) premultiplied r, g, b and opacity (1 on a hit, 0 otherwise) of an ``isosurface`` result under a headlight:
    colour * (ka + kd |n.d|) + ks |n.d|^shininess, two-sided, d the unit viewing direction.  A hit without a normal
    (zero gradient, normals=False) gets the ambient term alone.  ``background`` puts the result over a colour."""
    dirs = dirs.to(hits.normal.dtype)
    if dirs.shape != hits.normal.shape:
        raise ValueError('dirs must be (R, 3) like the hits, got %s' % (tuple(dirs.shape),))
    d = dirs / dirs.norm(dim=1, keepdim=True)
    c = (hits.normal * d).sum(1, keepdim=True).abs()
    col = torch.as_tensor(colour, dtype=c.dtype, device=c.device).reshape(1, 3)
    rgb = col * (float(ka) + float(kd) * c) + float(ks) * c ** float(shininess)
    alpha = hits.hit.to(c.dtype).view(-1, 1)
    return torch.cat([rgb * alpha, alpha], 1)


def surface_deviation(hits_a: IsoHits, hits_b: IsoHits) -> dict:
    """How far two ``isosurface`` results of the same rays are apart -- the surface counterpart of ``image_psnr``:
    'mismatch' (fraction of rays that hit in exactly one of the two), 'common' (rays that hit in both), and over those
    'depth_rms', 'depth_max' (of t_a - t_b, absolute) and 'angle_mean', 'angle_max' (degrees between the normals; rays
    with a zero normal in either result are left out of the angles).  All zero where there is nothing to compare."""
    if hits_a.hit.shape != hits_b.hit.shape:
        raise ValueError('the two results differ in their number of rays')
    both = hits_a.hit & hits_b.hit
    R, n = hits_a.hit.numel(), int(both.sum())
    out = {'mismatch': float((hits_a.hit ^ hits_b.hit).sum()) / R if R else 0.0, 'common': n,
           'depth_rms': 0.0, 'depth_max': 0.0, 'angle_mean': 0.0, 'angle_max': 0.0}
    if n:
        dt_ = (hits_a.t[both].double() - hits_b.t[both].double()).abs()
        out['depth_rms'], out['depth_max'] = float((dt_ ** 2).mean().sqrt()), float(dt_.max())
        na, nb = hits_a.normal[both].double(), hits_b.normal[both].double()
        ok = (na.norm(dim=1) > 0) & (nb.norm(dim=1) > 0)
        if bool(ok.any()):
            na, nb = na[ok], nb[ok]
            # atan2 of |a x b| and a . b: exact zero for equal normals, accurate at small angles (acos is neither)
            ang = torch.rad2deg(torch.atan2(torch.linalg.cross(na, nb).norm(dim=1), (na * nb).sum(1)))
            out['angle_mean'], out['angle_max'] = float(ang.mean()), float(ang.max())
    return out
