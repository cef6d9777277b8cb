"""Isosurface triangle meshes of the compressed model: the level set {value == iso} as vertices and triangles, extracted
on the device without reconstructing the volume on the host.  The reference exports the dense volume only.

    mesh = isosurface_mesh_from_net(dataset, net, iso=0.2, refine_steps=4)       # IsoMesh: vertices, triangles, normals, ...
    write_vtk_polydata(mesh, 'surface.vtk')                                       # opens in ParaView
    print(mesh_area(mesh), mesh_value_residual(mesh, dataset, volume))

Marching tetrahedra on the Kuhn triangulation of the volume lattice: every cell is cut into the same six tetrahedra, so
neighbouring cells agree on every shared face and the mesh is watertight by construction; there are no ambiguous cases
and the case table fits on a page (include/lfgc.h states the rule, tests/mesh_ref.py generates the table from it).  Every
lattice edge of the seven types -- three axis edges, three face diagonals, the body diagonal -- whose ends lie on
different sides of ``iso`` carries one vertex; vertices are ordered by (x, y, z, type) of the edge's lower end, triangles
by cell and tetrahedron.  Triangle normals point out of {value >= iso}, towards lower values.

The loop streams x-slabs: lattice values of the slab (one launch of the fused forward in lattice mode) ->
ops.iso_mesh_count -> read the two totals -> ops.iso_mesh_emit -> the bisection and the secant step of the ray caster
(ops.ray_iso_refine, ops.ray_iso_finish) along the lattice edges -> normals at the vertices.  The 16-byte read-back of
the totals per slab is the only synchronisation, and the mesh does not depend on the slab size in a single bit.  There
is no CPU form of the extraction: CPU tensors raise LfgcError.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import ops
from .._lib import LfgcError
from . import Render
from .OutputToVTK import field_from_net_fused, index_units_factor


class IsoMesh(NamedTuple):
    """Result of ``isosurface_mesh``: V vertices, T triangles."""
    vertices: torch.Tensor             # (V, 3) fp32, normalised coordinates
    triangles: torch.Tensor            # (T, 3) int32 vertex indices; (q1 - q0) x (q2 - q0) points out of {value >= iso}
    normals: Optional[torch.Tensor]    # (V, 3) unit normals -g / |g| (zero for a zero gradient), or None with normals=False
    values: torch.Tensor               # (V,) the value function at the vertices
    edge_lo: torch.Tensor              # (V, 3) the lattice position the vertex's edge starts at (its owner)
    edge_hi: torch.Tensor              # (V, 3) edge_lo + the edge's direction as the kernels hold it: the other lattice end
    bracket: torch.Tensor              # (V, 4) t_lo, t_hi, f_lo, f_hi as the bisection left them: the vertex sits at
    #                                    edge_lo + t (edge_hi - edge_lo) with t_lo <= t <= t_hi, f = value - iso at the ends
    iso: float


def _check(iso, refine_steps, res, max_slab_voxels):
    iso, n_refine = Render._iso_args(iso, refine_steps)
    res = tuple(int(v) for v in res)
    if len(res) != 3 or min(res) < 2:
        raise ValueError('the lattice needs three extents of at least 2, got %s' % (res,))
    planes = int(max_slab_voxels) // (res[1] * res[2])
    if planes < 3:
        raise ValueError('max_slab_voxels = %d holds fewer than three planes of %d x %d voxels' % (max_slab_voxels, res[1], res[2]))
    return iso, n_refine, res, planes


def isosurface_mesh(value_slab_fn: Callable, point_fn: Callable, res: Sequence[int], axis_tables, iso: float,
                    refine_steps: int = 0, normals: bool = True, max_slab_voxels: int = 1 << 24,
                    stats: Optional[dict] = None) -> IsoMesh:
    """The mesh of {value == iso} over the lattice ``res`` = (X, Y, Z).

    ``value_slab_fn(x_begin, x_end)`` returns the lattice values of those x-planes, (x_end - x_begin, Y, Z) fp32 on the
    device.  ``axis_tables`` = (xs (X,), ys (Y,), zs (Z,)) are the coordinates of the lattice points, separable per axis.
    ``point_fn(pos (n, 3))`` returns the values at arbitrary points; it is called ``refine_steps`` times per slab with one
    trial point per vertex, once more at the final vertices, and with ``normals=True`` that last call is
    ``point_fn(pos, gradient=True)`` and must return (values, gradients (n, 3)).

    A vertex sits on its lattice edge where the secant through the bracket's end values crosses ``iso`` (linear
    interpolation, clamped to the edge; the midpoint when the quotient is not finite).  With ``refine_steps = k`` the
    bracket is first bisected k times with values of ``point_fn``, so the vertex lies within 2^-k of the edge's length of a
    root of the value function itself rather than of its lattice interpolant.  A vertex on a lattice point gives zero-area
    triangles; they are kept, the connectivity stays manifold.

    A slab holds at most ``max_slab_voxels`` lattice values (at least three planes); its last two planes are only read,
    to rank the edges its last cells reference, and the next slab starts there.  A mesh that reaches 2^31 vertices is
    refused.  ``stats`` receives 'slabs' and 'point_samples' (rows evaluated by point_fn)."""
    iso, n_refine, res, planes = _check(iso, refine_steps, res, max_slab_voxels)
    xs, ys, zs = axis_tables
    if (xs.numel(), ys.numel(), zs.numel()) != res:
        raise ValueError('axis tables of %d, %d, %d entries for a lattice of %s' % (xs.numel(), ys.numel(), zs.numel(), res))
    ops._require_hip(xs, ys, zs)
    xs, ys, zs = ops._f32c(xs.detach()), ops._f32c(ys.detach()), ops._f32c(zs.detach())
    dev = xs.device
    X = res[0]
    parts = {k: [] for k in ('vertices', 'triangles', 'normals', 'values', 'edge_lo', 'edge_hi', 'bracket')}
    n_vertices, n_slabs, n_samples, x0 = 0, 0, 0, 0
    while x0 < X:
        x1, xe = (X, X) if X - x0 <= planes else (x0 + planes - 2, x0 + planes)
        vals = value_slab_fn(x0, xe)
        ops._require_hip(vals)
        vals = ops._f32c(vals.detach())
        if tuple(vals.shape) != (xe - x0, res[1], res[2]):
            raise ValueError('value_slab_fn(%d, %d) returned %s, expected %s' % (x0, xe, tuple(vals.shape), (xe - x0, res[1], res[2])))
        ws, V, T = ops.iso_mesh_count(vals, x1 - x0, iso)
        if n_vertices + V >= 2 ** 31:
            raise ValueError('the mesh reaches 2^31 vertices: triangle indices are int32')
        origins, dirs, bracket, tris = ops.iso_mesh_emit(vals, x1 - x0, iso, xs[x0:xe], ys, zs, n_vertices, ws, V, T)
        every = torch.arange(V, dtype=torch.int32, device=dev)
        _, pos = Render._refine_and_finish(point_fn, every, origins, dirs, iso, bracket, n_refine if V else 0)
        if not V:                                                                   # nothing to evaluate: empty rows
            out = torch.empty(0, dtype=torch.float32, device=dev)
            if normals:
                parts['normals'].append(torch.empty((0, 3), dtype=torch.float32, device=dev))
        elif normals:
            out, g = Render._values_and_gradients(point_fn(pos, gradient=True), 'point_fn')
            parts['normals'].append(Render._unit(-g))           # -g / |g|, +0 for a zero gradient
        else:
            out = point_fn(pos)
        parts['values'].append(out.reshape(-1).to(torch.float32))
        for k, a in (('vertices', pos), ('triangles', tris), ('edge_lo', origins), ('edge_hi', origins + dirs), ('bracket', bracket)):
            parts[k].append(a)
        n_vertices += V
        n_samples += (n_refine + 1) * V
        n_slabs += 1
        x0 = x1
    if stats is not None:
        stats.update(slabs=n_slabs, point_samples=n_samples)
    cat = {k: torch.cat(v) for k, v in parts.items() if v}
    return IsoMesh(cat['vertices'], cat['triangles'], cat.get('normals'), cat['values'], cat['edge_lo'], cat['edge_hi'],
                   cat['bracket'], iso)


def lattice_axis_tables(res, scales, device, tiled_res: int = 32):
    """(xs, ys, zs): the normalised coordinates of the volume lattice per axis, as ops.lattice_slab_positions -- and with it
    the fused forward in lattice mode -- forms them tile by tile.  They are separable: a coordinate depends on its own
    index, its own extent and scale only, so each table is read off a lattice that is two voxels thin in the other axes."""
    tables = []
    for a in range(3):
        thin = [2, 2, 2]
        thin[a] = int(res[a])
        pos = ops.lattice_slab_positions(thin, 0, thin[0], tiled_res, scales, device).view(thin[0], thin[1], thin[2], 3)
        index = [0, 0, 0]
        index[a] = slice(None)
        tables.append(pos[index[0], index[1], index[2], a].contiguous())
    return tuple(tables)


def isosurface_mesh_from_net(dataset, net, iso: float, tiled_res: int = 32, **kwargs) -> IsoMesh:
    """``isosurface_mesh`` of the compressed model over the dataset's volume lattice.  Slab values: ``field_from_net_fused``
    (the clamped eval-mode output, so ``iso`` must lie strictly inside (-1, 1)); trial points: ops.forward_raw with the
    clamp, as the ray caster evaluates them; normals: ``net.value_and_gradient`` in eval mode; lattice coordinates:
    ``lattice_axis_tables``, the positions the lattice kernel uses.  Honours ``net.precision``."""
    if not -1.0 < float(iso) < 1.0:
        raise ValueError('iso must lie inside the clamp range (-1, 1) of the eval-mode output, got %r' % (iso,))
    res = dataset.vol_res_touple
    _check(iso, kwargs.get('refine_steps', 0), res, kwargs.get('max_slab_voxels', 1 << 24))
    first = next(iter(net.parameters()), None)
    dev = first.device if first is not None else torch.device('cpu')
    if dev.type != 'cuda':
        raise LfgcError('the mesh is extracted on the MI355X only: the model is on %s; there is no CPU fallback.' % dev)
    if kwargs.get('normals', True) and net.training:
        raise ValueError('normals come from net.value_and_gradient in eval mode: call net.eval() first')
    tables = lattice_axis_tables(res, dataset.scales.tolist(), dev, tiled_res)

    def value_slab_fn(x_begin, x_end):
        return field_from_net_fused(dataset, net, x_begin, x_end, tiled_res)
    return isosurface_mesh(value_slab_fn, Render._net_value_fn(net), res, tables, iso, **kwargs)


def volume_axis_tables(dataset, device):
    """(xs, ys, zs): the normalised coordinates of the voxels per axis, IndexDataset.positions_for of the indices."""
    tables = []
    for a, n in enumerate(dataset.vol_res_touple):
        raw = torch.zeros((n, 3), dtype=torch.float32)
        raw[:, a] = torch.arange(n, dtype=torch.float32)
        tables.append(dataset.positions_for(raw)[1][:, a].contiguous().to(device))
    return tuple(tables)


def isosurface_mesh_from_volume(dataset, volume: torch.Tensor, iso: float, **kwargs) -> IsoMesh:
    """The same loop over the ground truth: the lattice values are the voxels, trial points are read with the trilinear
    sampler (ops.gt_interp of ``index_positions``), normals are its central differences (Render.volume_value_fn).  Same
    lattice, same iso as ``isosurface_mesh_from_net`` -> ``mesh_value_residual`` measures one surface against the other."""
    res = dataset.vol_res_touple
    _check(iso, kwargs.get('refine_steps', 0), res, kwargs.get('max_slab_voxels', 1 << 24))
    ops._require_hip(volume)
    volume = ops._f32c(volume.detach())
    if tuple(volume.shape) != tuple(res):
        raise ValueError('volume is %s, the dataset %s' % (tuple(volume.shape), res))
    return isosurface_mesh(lambda b, e: volume[b:e], Render.volume_value_fn(dataset, volume), res,
                           volume_axis_tables(dataset, volume.device), iso, **kwargs)


# ---- measures (pure torch: these also run on the CPU) -----------------------------------------------------------------------

def mesh_area(mesh: IsoMesh) -> float:
    """Sum of the triangle areas, accumulated in float64."""
    q = mesh.vertices.double()[mesh.triangles.long()]
    return 0.5 * float(torch.linalg.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]).norm(dim=1).sum())


def _trilinear_host(idx_pos: torch.Tensor, volume: torch.Tensor) -> torch.Tensor:
    """Trilinear interpolation of ``volume`` at positions in index units inside the volume (float64; host tensors)."""
    p = idx_pos.double()
    hi = torch.tensor([s - 1 for s in volume.shape], dtype=torch.float64)
    i0 = torch.minimum(p.floor().clamp(min=0), (hi - 1).clamp(min=0))
    f = p - i0
    i0 = i0.long()
    i1 = torch.minimum(i0 + 1, hi.long())
    v = volume.double()
    out = torch.zeros(p.shape[0], dtype=torch.float64)
    for c in range(8):
        sel = [(i1 if c >> (2 - a) & 1 else i0)[:, a] for a in range(3)]
        w = torch.ones_like(out)
        for a in range(3):
            w = w * (f[:, a] if c >> (2 - a) & 1 else 1.0 - f[:, a])
        out += w * v[sel[0], sel[1], sel[2]]
    return out.to(torch.float32)


def mesh_value_residual(mesh: IsoMesh, dataset, volume: torch.Tensor) -> dict:
    """How far the mesh lies from the ground truth's level set -- the mesh counterpart of ``surface_deviation``: 'rms' and
    'max' of gt(vertex) - iso over the vertices, and 'distance_rms', 'distance_max': the same divided by the magnitude of
    the ground truth's gradient (central differences), a first-order distance, in voxels.  Vertices where that gradient
    vanishes are left out of the distances.  All zero for an empty mesh.  Device tensors use ops.gt_interp; host tensors a
    float64 torch form of the same sampler."""
    out = {'rms': 0.0, 'max': 0.0, 'distance_rms': 0.0, 'distance_max': 0.0}
    if mesh.vertices.shape[0] == 0:
        return out
    on_device = volume.is_cuda
    fn = Render.volume_value_fn(dataset, volume, None if on_device else _trilinear_host)
    v, g = fn(mesh.vertices.to(volume.device), gradient=True)
    r = (v.double() - float(mesh.iso)).abs()
    out['rms'], out['max'] = float((r ** 2).mean().sqrt()), float(r.max())
    gn = g.double().norm(dim=1) * index_units_factor(dataset)                   # per voxel step
    ok = gn > 0
    if bool(ok.any()):
        d = r[ok] / gn[ok]
        out['distance_rms'], out['distance_max'] = float((d ** 2).mean().sqrt()), float(d.max())
    return out


# ---- file output ----------------------------------------------------------------------------------------------------------------

def write_vtk_polydata(mesh: IsoMesh, filename: str, binary: bool = True, title: str = 'isosurface') -> None:
    """Legacy VTK ``POLYDATA`` file of the mesh (ParaView, VisIt): POINTS, POLYGONS and, as POINT_DATA, the scalar ``value``
    and -- when the mesh has them -- NORMALS.  ``binary=True`` writes big-endian payloads, as the format demands."""
    pts = mesh.vertices.detach().cpu().numpy().astype(np.float32)
    tri = mesh.triangles.detach().cpu().numpy().astype(np.int32)
    val = mesh.values.detach().cpu().numpy().astype(np.float32)
    nrm = None if mesh.normals is None else mesh.normals.detach().cpu().numpy().astype(np.float32)
    V, T = pts.shape[0], tri.shape[0]
    cells = np.concatenate([np.full((T, 1), 3, np.int32), tri], 1)

    def payload(f, a, fmt):
        if binary:
            f.write(np.ascontiguousarray(a).astype(a.dtype.newbyteorder('>')).tobytes())
            f.write(b'\n')
        else:
            for row in a.reshape(a.shape[0], -1):
                f.write((' '.join(fmt % x for x in row) + '\n').encode('ascii'))

    with open(filename, 'wb') as f:
        f.write(('# vtk DataFile Version 3.0\n%s\n%s\nDATASET POLYDATA\n' % (title.replace('\n', ' ')[:255],
                                                                             'BINARY' if binary else 'ASCII')).encode('ascii'))
        f.write(('POINTS %d float\n' % V).encode('ascii'))
        payload(f, pts, '%.9g')
        f.write(('POLYGONS %d %d\n' % (T, 4 * T)).encode('ascii'))
        payload(f, cells, '%d')
        f.write(('POINT_DATA %d\nSCALARS value float 1\nLOOKUP_TABLE default\n' % V).encode('ascii'))
        payload(f, val.reshape(-1, 1), '%.9g')
        if nrm is not None:
            f.write(b'NORMALS normals float\n')
            payload(f, nrm, '%.9g')
