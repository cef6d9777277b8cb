"""Host-side tests of the isosurface mesh extraction (no GPU): the NumPy restatement (tests/mesh_ref.py) against closed
forms and against itself run slab-wise, the new C entries in the header, the binding and the kernel's case table, the
argument checks that run before any launch, the VTK writer, the two measures on a hand-made mesh, and -- with the oracle --
the conditions the GPU test of the network case relies on."""
import math
import os
import re
import struct

import numpy as np
import pytest
import torch

import mesh_ref as MR
from latent_feature_grid_compression_amd import _lib, ops
from latent_feature_grid_compression_amd._lib import LfgcError
from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
from latent_feature_grid_compression_amd.visualization import Mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('lfgc_iso_mesh_workspace_bytes', 'lfgc_iso_mesh_count_f32', 'lfgc_iso_mesh_emit_f32')


# ---- the restatement against mathematics -------------------------------------------------------------------------------

@pytest.mark.parametrize('field, shape, chi', [(MR.sphere_field, (13, 12, 11), 2), (MR.torus_field, (17, 18, 9), 0),
                                               (MR.two_spheres_field, (21, 9, 9), 4)])
def test_closed_surfaces_are_closed_oriented_and_have_their_euler_characteristic(field, shape, chi):
    tabs, P = MR.lattice(shape)
    m = MR.mesh(field(P), *tabs, 0.0)
    V, T = len(m['vertices']), m['triangles']
    assert V > 100 and T.min() == 0 and T.max() == V - 1
    assert MR.is_closed(T) and MR.is_oriented(T)
    assert MR.euler_characteristic(V, T) == chi
    if field is MR.sphere_field:
        assert (V, len(T)) == (838, 1672)                        # the counts of the rule's prototype on this lattice


def test_sphere_normals_point_away_from_the_centre():
    tabs, P = MR.lattice((13, 12, 11))
    m = MR.mesh(MR.sphere_field(P), *tabs, 0.0)
    n = MR.triangle_normals(m['vertices'], m['triangles'])
    centroid = m['vertices'].astype(np.float64)[m['triangles']].mean(1)
    out = ((centroid - MR.SPHERE_C) * n).sum(1)
    area2 = np.linalg.norm(n, axis=1)
    assert (out[area2 > 1e-9] > 0).all() and (area2 > 1e-9).mean() > 0.95


def test_sphere_area_at_25_cubed():
    tabs, P = MR.lattice((25, 25, 25))
    m = MR.mesh(MR.sphere_field(P), *tabs, 0.0)
    want = 4 * math.pi * MR.SPHERE_R ** 2
    assert abs(MR.area(m['vertices'], m['triangles']) - want) <= 0.03 * want


@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_plane_area_is_the_cross_section_of_the_box(sign):
    """v = +-(z - c) is linear along every edge, so the secant step lands on the plane up to float32 rounding and the
    triangles tile the 2 x 2 cross-section; the winding follows the side that is inside."""
    c = 0.137
    tabs, P = MR.lattice((7, 9, 11))
    m = MR.mesh((sign * (P[..., 2] - c)).astype(np.float32), *tabs, 0.0)
    assert np.abs(m['vertices'][:, 2] - c).max() <= 4 * 2.0 ** -24
    assert abs(MR.area(m['vertices'], m['triangles']) - 4.0) <= 1e-5
    n = MR.triangle_normals(m['vertices'], m['triangles'])
    assert (n[:, 2] * -sign > 0).all()                            # out of {v >= 0}: towards lower values


@pytest.mark.parametrize('shape, seed', [((5, 6, 7), 1), ((9, 4, 8), 2), ((2, 2, 2), 3), ((2, 5, 3), 4)])
def test_random_fields_are_manifold_with_boundary_on_the_lattice_faces(shape, seed):
    v, tabs, iso = MR.random_case(shape, seed)
    m = MR.mesh(v, *tabs, iso)
    T = m['triangles']
    assert len(T) > 0
    assert all(n == 1 for n in MR.directed_edges(T).values())                  # each direction at most once
    und = MR.undirected_edges(T)
    assert set(und.values()) <= {1, 2}
    lo, hi = [t[0] for t in tabs], [t[-1] for t in tabs]
    for (a, b), n in und.items():
        if n == 1:                                                              # a boundary edge lies in a face of the lattice
            pa, pb = m['vertices'][a], m['vertices'][b]
            assert any((pa[k] == lo[k] and pb[k] == lo[k]) or (pa[k] == hi[k] and pb[k] == hi[k]) for k in range(3)), (a, b)
    assert np.isfinite(m['vertices']).all()                                     # a NaN end gives the edge's midpoint


def test_inside_rule_and_vertex_order():
    """v == iso is inside, a NaN is not; vertices ascend in (x, y, z, ty) of the owner; the bracket is (0, 1, f_lo, f_hi)."""
    v = np.full((2, 2, 2), -1.0, np.float32)
    v[0, 0, 0] = 0.25
    v[1, 1, 1] = np.nan
    tabs = [np.array([0.0, 1.0], np.float32), np.array([0.0, 2.0], np.float32), np.array([0.0, 4.0], np.float32)]
    assert MR.count(v, 2, 0.25) == (7, 6)                                       # corner 0 alone inside: 7 edges, one triangle per tet
    o, d, br, tr = MR.emit(v, 2, 0.25, *tabs, 10)
    assert np.array_equal(o, np.zeros((7, 3), np.float32))
    assert np.array_equal(d, MR.OFFSETS[1:] * np.array([1.0, 2.0, 4.0], np.float32))
    assert np.array_equal(br[:6], np.tile(np.array([0, 1, 0, -1.25], np.float32), (6, 1))) and np.isnan(br[6, 3])
    assert tr.min() == 10 and tr.max() == 16 and tr.shape == (6, 3)
    # every triangle holds the body diagonal's vertex (type 7) and two of the others
    assert ((tr == 16).sum(1) == 1).all()


@pytest.mark.parametrize('refine_steps', [0, 3])
def test_slabs_do_not_show(refine_steps):
    tabs, P = MR.lattice((13, 12, 11))
    field = MR.sphere_field(P)

    def value_of(p):
        return (MR.SPHERE_R - np.linalg.norm(np.asarray(p, np.float64) - MR.SPHERE_C, axis=1)).astype(np.float32)
    whole = MR.mesh(field, *tabs, 0.0, refine_steps, value_of)
    for owner in (1, 2, 5):
        assert len(MR.slabs(13, owner)) > 1
        part = MR.mesh(field, *tabs, 0.0, refine_steps, value_of, owner_planes=owner)
        for k in whole:
            assert np.array_equal(whole[k], part[k], equal_nan=True), (owner, k)
    v, rtabs, iso = MR.random_case((9, 4, 8), 7)
    whole = MR.mesh(v, *rtabs, iso)
    for owner in (1, 2, 5):
        part = MR.mesh(v, *rtabs, iso, owner_planes=owner)
        for k in whole:
            assert np.array_equal(whole[k], part[k], equal_nan=True), (owner, k)
    assert MR.slabs(13, 5) == [(0, 5, 7), (5, 10, 12), (10, 13, 13)] and MR.slabs(8, 1) [-1] == (5, 8, 8)


def test_refinement_converges_on_the_sphere():
    """With the value function itself the vertices lie on the sphere: 2^-k of the longest edge bounds the distance."""
    tabs, P = MR.lattice((13, 12, 11))

    def value_of(p):
        return (MR.SPHERE_R - np.linalg.norm(np.asarray(p, np.float64) - MR.SPHERE_C, axis=1)).astype(np.float32)
    err = []
    for k in (0, 6):
        m = MR.mesh(MR.sphere_field(P), *tabs, 0.0, k, value_of)
        err.append(np.abs(np.linalg.norm(m['vertices'].astype(np.float64) - MR.SPHERE_C, axis=1) - MR.SPHERE_R).max())
    longest = math.sqrt((2 / 12) ** 2 + (2 / 11) ** 2 + (2 / 10) ** 2)
    assert err[1] <= longest * 2.0 ** -6 and err[1] < err[0] / 16


# ---- header, binding, case table -------------------------------------------------------------------------------------------

def test_entries_are_declared_and_bound_with_matching_arity():
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'lfgc.h')).read(), flags=re.S)
    for name in ENTRIES:
        m = re.search(r'\b(int|int64_t)\s+%s\s*\(([^)]*)\)\s*;' % name, header)
        assert m, '%s is not declared in include/lfgc.h' % name
        params = [p for p in m.group(2).split(',') if p.strip()]
        assert name in _lib.SIGNATURES, '%s is not bound in _lib.py' % name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is (_lib.c_int if m.group(1) == 'int' else _lib.c_int64)
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        if m.group(1) == 'int':
            assert params[-1].split()[0] == 'lfgc_stream_t'
    assert callable(ops.iso_mesh_count) and callable(ops.iso_mesh_emit)
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(name in text for name in ENTRIES)


def test_library_exports_the_entries():
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        getattr(lib, name)


def test_the_kernels_case_table_is_the_generated_one():
    src = open(os.path.join(ROOT, 'latent_feature_grid_compression_amd', 'csrc', 'lfgc_mesh.hip')).read()
    body = src[src.index('kCase[96] = {'):]
    body = body[:body.index('};')]
    words = [int(w, 16) for w in re.findall(r'0x([0-9a-f]+)ull', body)]
    want = [MR.pack_case(t) for row in MR.CASES for t in row]
    assert words == want
    for k, row in enumerate(MR.CASES):                                # the rule's counts: 0, 1 or 2 triangles by the mask's bit count
        for m, tris in enumerate(row):
            assert len(tris) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[bin(m).count('1')]
            for t in tris:
                assert all(1 <= ty <= 7 and c in MR.tet_corners(k) and (c | ty) in MR.tet_corners(k) for c, ty in t)


def test_workspace_query_and_argument_errors_before_any_launch():
    """No device is touched: every refusal below is decided on the host, with null or bogus pointers in place."""
    lib = _lib.load()
    assert lib.lfgc_iso_mesh_workspace_bytes(0, 1, 4, 4) == 16 and lib.lfgc_iso_mesh_workspace_bytes(4, 5, 4, 4) == 16
    small, big = lib.lfgc_iso_mesh_workspace_bytes(4, 2, 5, 6), lib.lfgc_iso_mesh_workspace_bytes(600, 598, 40, 40)
    assert small >= 2048 * 10 and small % 16 == 0 and big >= 599 * 1600 * 10 and big > small
    assert lib.lfgc_iso_mesh_workspace_bytes(7, 2, 5, 6) == lib.lfgc_iso_mesh_workspace_bytes(3, 2, 5, 6)      # 3 planes are ranked
    p = 4096                                                          # a non-null, 16-byte aligned value that is never dereferenced
    NULL, SHAPE, UNSUPPORTED, ALIGN, WORKSPACE = -1, -2, -3, -4, -5
    count = lib.lfgc_iso_mesh_count_f32
    assert count(None, 4, 2, 5, 6, 0.0, p, p, small, None) == NULL
    assert count(p, 4, 2, 5, 6, 0.0, None, p, small, None) == NULL
    assert count(p, 4, 2, 5, 6, 0.0, p, None, small, None) == NULL
    for nx, n_owner, ny, nz in ((0, 1, 5, 6), (4, 0, 5, 6), (4, 5, 5, 6), (4, 2, 1, 6), (4, 2, 5, 1)):
        assert count(p, nx, n_owner, ny, nz, 0.0, p, p, small, None) == SHAPE
    assert count(p, 4, 2, 5, 6, float('nan'), p, p, small, None) == SHAPE
    assert count(p, 4, 2, 5, 6, float('inf'), p, p, small, None) == SHAPE
    assert count(p, 1024, 1022, 512, 512, 0.0, p, p, 1 << 40, None) == UNSUPPORTED
    assert count(p, 4, 2, 5, 6, 0.0, p, p + 8, small, None) == ALIGN
    assert count(p, 4, 2, 5, 6, 0.0, p, p, small - 1, None) == WORKSPACE
    emit = lib.lfgc_iso_mesh_emit_f32
    args = lambda **kw: [kw.get(k, d) for k, d in (('values', p), ('nx', 4), ('n_owner', 2), ('ny', 5), ('nz', 6), ('iso', 0.0),    # noqa: E731
                                                   ('xs', p), ('ys', p), ('zs', p), ('base', 0), ('ws', p), ('ws_bytes', small),
                                                   ('nv', 3), ('nt', 3), ('origins', p), ('dirs', p), ('bracket', p),
                                                   ('triangles', p), ('stream', None))]
    assert emit(*args(nv=0, nt=0, values=None)) == 0                  # nothing to emit returns at once
    for k in ('values', 'xs', 'ys', 'zs', 'ws', 'origins', 'dirs', 'bracket', 'triangles'):
        assert emit(*args(**{k: None})) == NULL, k
    assert emit(*args(nv=0, origins=None, dirs=None, bracket=None, nx=0)) == SHAPE       # outputs of an empty part may be null
    for bad in (dict(nx=0), dict(n_owner=5), dict(ny=1), dict(nz=1), dict(iso=float('nan')), dict(base=-1), dict(base=1 << 31),
                dict(nv=-1), dict(nt=-1)):
        assert emit(*args(**bad)) == SHAPE, bad
    assert emit(*args(bracket=p + 4)) == ALIGN and emit(*args(ws=p + 8)) == ALIGN
    assert emit(*args(ws_bytes=small - 1)) == WORKSPACE


def test_isosurface_mesh_arguments_are_checked_before_anything_runs():
    calls = []
    slab = lambda b, e: calls.append((b, e))                      # noqa: E731
    point = lambda p, gradient=False: calls.append(p)             # noqa: E731
    tabs = [torch.linspace(-1, 1, n) for n in (4, 5, 6)]
    ok = dict(res=(4, 5, 6), axis_tables=tabs, iso=0.0)
    for bad in (dict(iso=float('nan')), dict(iso=float('inf')), dict(refine_steps=-1), dict(refine_steps=65), dict(refine_steps=1.5),
                dict(res=(1, 5, 6)), dict(res=(4, 5, 1)), dict(res=(4, 5)), dict(max_slab_voxels=89), dict(res=(4, 5, 7))):
        with pytest.raises(ValueError):
            Mesh.isosurface_mesh(slab, point, **{**ok, **bad})
    with pytest.raises(LfgcError):                                  # three planes fit, the arguments are fine: CPU tensors
        Mesh.isosurface_mesh(slab, point, max_slab_voxels=90, **ok)
    assert not calls
    ds = IndexDataset((4, 5, 6), build_index_table=False)
    net = torch.nn.Linear(3, 1)
    for bad in (-1.0, 1.0, float('nan')):
        with pytest.raises(ValueError):
            Mesh.isosurface_mesh_from_net(ds, net, bad)
    with pytest.raises(ValueError):
        Mesh.isosurface_mesh_from_net(ds, net, 0.0, refine_steps=70)
    with pytest.raises(LfgcError):
        Mesh.isosurface_mesh_from_net(ds, net, 0.0)
    with pytest.raises(ValueError):
        Mesh.isosurface_mesh_from_volume(ds, torch.zeros(4, 5, 6), float('inf'))
    with pytest.raises(LfgcError):
        Mesh.isosurface_mesh_from_volume(ds, torch.zeros(4, 5, 6), 0.0)
    v = torch.zeros(4, 5, 6)
    with pytest.raises(LfgcError):
        ops.iso_mesh_count(v, 2, 0.0)
    with pytest.raises(LfgcError):
        ops.iso_mesh_emit(v, 2, 0.0, *tabs, 0, torch.zeros(8, dtype=torch.int64), 0, 0)


# ---- the VTK writer and the measures on a hand-made mesh ---------------------------------------------------------------------

def _two_triangles(normals=True):
    """The unit square in the plane z = 0.25 of a (5, 5, 5) volume's box, as two triangles facing +z."""
    vert = torch.tensor([[0.0, 0, 0.25], [1.0, 0, 0.25], [1.0, 1.0, 0.25], [0.0, 1.0, 0.25]])
    tri = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    nrm = torch.tensor([[0.0, 0, 1.0]] * 4) if normals else None
    val = torch.tensor([0.5, 0.25, -0.125, 3.0])
    z = torch.zeros(4, 3)
    return Mesh.IsoMesh(vert, tri, nrm, val, z, z, torch.zeros(4, 4), 0.3)


def _parse_vtk(path):
    """A reader of just what write_vtk_polydata writes: (title, kind, points, polygons, value, normals or None)."""
    data = open(path, 'rb').read()
    pos = 0

    def line():
        nonlocal pos
        end = data.index(b'\n', pos)
        out, pos = data[pos:end].decode('ascii'), end + 1
        return out

    def block(count, code, size):
        nonlocal pos
        if kind == 'BINARY':
            out = struct.unpack('>%d%s' % (count, code), data[pos:pos + count * size])
            pos += count * size
            assert data[pos:pos + 1] == b'\n'
            pos += 1
            return list(out)
        out = []
        while len(out) < count:
            out += [float(t) if code == 'f' else int(t) for t in line().split()]
        return out
    assert line() == '# vtk DataFile Version 3.0'
    title, kind = line(), line()
    assert kind in ('BINARY', 'ASCII') and line() == 'DATASET POLYDATA'
    word, n, typ = line().split()
    assert word == 'POINTS' and typ == 'float'
    n = int(n)
    points = np.array(block(3 * n, 'f', 4), np.float32).reshape(n, 3)
    word, t, size = line().split()
    assert word == 'POLYGONS' and int(size) == 4 * int(t)
    polys = np.array(block(int(size), 'i', 4), np.int32).reshape(int(t), 4)
    assert line() == 'POINT_DATA %d' % n and line() == 'SCALARS value float 1' and line() == 'LOOKUP_TABLE default'
    value = np.array(block(n, 'f', 4), np.float32)
    normals = None
    if pos < len(data):
        assert line() == 'NORMALS normals float'
        normals = np.array(block(3 * n, 'f', 4), np.float32).reshape(n, 3)
    assert pos == len(data)
    return title, kind, points, polys, value, normals


@pytest.mark.parametrize('binary', [True, False])
@pytest.mark.parametrize('normals', [True, False])
def test_write_vtk_polydata_round_trips(tmp_path, binary, normals):
    mesh = _two_triangles(normals)
    path = str(tmp_path / 'mesh.vtk')
    Mesh.write_vtk_polydata(mesh, path, binary=binary, title='two triangles')
    title, kind, points, polys, value, nrm = _parse_vtk(path)
    assert title == 'two triangles' and kind == ('BINARY' if binary else 'ASCII')
    assert np.array_equal(points, mesh.vertices.numpy())           # %.9g round-trips a float32
    assert np.array_equal(polys, np.array([[3, 0, 1, 2], [3, 0, 2, 3]], np.int32))
    assert np.array_equal(value, mesh.values.numpy())
    assert (nrm is None) == (not normals) and (nrm is None or np.array_equal(nrm, mesh.normals.numpy()))
    if binary:                                                      # big-endian: 1.0f is 3f 80 00 00 right after the POINTS line
        raw = open(path, 'rb').read()
        at = raw.index(b'POINTS 4 float\n') + len(b'POINTS 4 float\n')
        assert raw[at + 12:at + 16] == b'\x3f\x80\x00\x00'


def test_mesh_area_and_value_residual_on_a_hand_made_mesh():
    mesh = _two_triangles()
    assert Mesh.mesh_area(mesh) == 1.0
    # a (5, 5, 5) volume whose value is 0.1 * (z index): index = 2 (pos + 1), so gt(vertex) = 0.1 * 2 * 1.25 = 0.25
    ds = IndexDataset((5, 5, 5), build_index_table=False)
    vol = (0.1 * torch.arange(5, dtype=torch.float32)).view(1, 1, 5).expand(5, 5, 5).contiguous()
    res = Mesh.mesh_value_residual(mesh, ds, vol)
    assert abs(res['rms'] - 0.05) <= 1e-6 and abs(res['max'] - 0.05) <= 1e-6          # |0.25 - iso|, iso = 0.3
    # the gradient is 0.1 per voxel, so the surface lies half a voxel away
    assert abs(res['distance_rms'] - 0.5) <= 1e-4 and abs(res['distance_max'] - 0.5) <= 1e-4
    empty = Mesh.IsoMesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), None, torch.zeros(0), torch.zeros(0, 3),
                         torch.zeros(0, 3), torch.zeros(0, 4), 0.0)
    assert Mesh.mesh_area(empty) == 0.0
    assert Mesh.mesh_value_residual(empty, ds, vol) == {'rms': 0.0, 'max': 0.0, 'distance_rms': 0.0, 'distance_max': 0.0}


# ---- conditions the GPU tests rely on, checked here with the oracle ----------------------------------------------------------

def test_gpu_lattices_give_vertices_and_triangles():
    for i, shape in enumerate(MR.GPU_LATTICES):
        v, tabs, iso = MR.random_case(shape, 100 + i)
        V, T = MR.count(v, shape[0], iso)
        assert V > 0 and T > 0 and np.isnan(v).any() and (v == np.float32(iso)).any()
        o, d, br, tr = MR.emit(v, shape[0], iso, *tabs, 0)
        assert (len(o), len(tr)) == (V, T) and tr.max() == V - 1


def test_network_case_conditions_by_the_oracle():
    case = MR.oracle_net_case()
    lat = case['lattice'].astype(np.float64)
    # no lattice value near iso: the device's inside bits cannot differ from the oracle's (forward parity bound 2e-5)
    assert np.abs(lat - MR.NET_ISO).min() >= MR.NET_NEAR
    share = (lat >= MR.NET_ISO).mean()
    assert 0.2 < share < 0.8
    coarse, fine = case['coarse'], case['fine']
    V, T = len(coarse['vertices']), coarse['triangles']
    assert V > 3000 and len(T) > 6000 and np.array_equal(T, fine['triangles'])
    assert MR.is_oriented(T) and set(MR.undirected_edges(T).values()) <= {1, 2}
    # six bisections and the secant step: the residual falls far below 1/16 (the GPU test's bound), by the oracle alone
    rms = [np.sqrt(np.mean((m['values'].astype(np.float64) - MR.NET_ISO) ** 2)) for m in (coarse, fine)]
    print('oracle: rms(value - iso) %.3e at 0 steps, %.3e at %d steps, ratio %.1f' % (rms[0], rms[1], MR.NET_REFINE, rms[0] / rms[1]))
    assert rms[1] < rms[0] / 64
    br = fine['bracket']
    assert ((br[:, 2] >= 0) != (br[:, 3] >= 0)).all() and (br[:, 1] - br[:, 0] <= 2.0 ** -MR.NET_REFINE).all()
    # normals -g / |g| agree with the winding on at least 99 % of the vertex-triangle incidences
    _, g = MR.oracle_net()(fine['vertices'], gradient=True)
    g = g.astype(np.float64)
    agree, n = MR.winding_agreement(fine['vertices'], T, -g / np.linalg.norm(g, axis=1, keepdims=True))
    print('oracle: normal . triangle normal > 0 on %.4f of %d incidences' % (agree, n))
    assert agree >= 0.995
