"""NumPy restatement of the isosurface mesh extraction's contract (include/lfgc.h) -- a helper, not a test.

Marching tetrahedra on the Kuhn triangulation of the volume lattice: the inside rule, the 7-bit crossing-edge flags, their
ranks and order, the 6 x 16 case table (GENERATED here from the geometric rule; the kernel's constexpr copy is what
``print_case_table`` prints), the triangles, and the whole slab loop of Mesh.isosurface_mesh with the bisection and the
secant step of iso_ref.  Every operation is an individually rounded float32 operation, so the device results are expected
to be EQUAL, not close.  Written from the contract, not from the kernels.  Also the topology helpers of the tests
(directed / undirected edge counts, Euler characteristic) and their shared inputs."""
import itertools

import numpy as np

import iso_ref as IR

F = np.float32

# edge type ty = 1..7 and cube corner c = 0..7 share one code: offset (c >> 2 & 1, c >> 1 & 1, c & 1) in (x, y, z)
OFFSETS = np.array([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(8)])
PERMS = tuple(itertools.permutations((0, 1, 2)))          # lexicographic: (0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0)


def tet_corners(k):
    """Cube corner codes (w0, w1, w2, w3) of tetrahedron k: w0 = (0,0,0), w1 = w0 + e[p0], w2 = w1 + e[p1], w3 = (1,1,1)."""
    p = PERMS[k]
    w1 = 4 >> p[0]
    return (0, w1, w1 | (4 >> p[1]), 7)


def _edge(w, a, b):
    """The mesh vertex on the edge between tetrahedron corners a and b: (owner cube corner, edge type)."""
    lo, hi = w[min(a, b)], w[max(a, b)]
    return (lo, hi ^ lo)                                   # hi contains lo bitwise: the difference is the offset code


def _midpoint(v):
    return OFFSETS[v[0]] + 0.5 * OFFSETS[v[1]]


def case_table():
    """table[k][m]: the triangles of tetrahedron k with inside mask m (bit n = inside(w_n)); a triangle is three mesh
    vertices (owner cube corner, edge type) in the emitted winding."""
    table = []
    for k in range(6):
        w = tet_corners(k)
        row = []
        for m in range(16):
            ins = [n for n in range(4) if m >> n & 1]
            out = [n for n in range(4) if not m >> n & 1]
            tris = []
            if len(ins) in (1, 3):
                a = (ins if len(ins) == 1 else out)[0]
                b, c, d = [n for n in range(4) if n != a]
                tris = [[_edge(w, a, b), _edge(w, a, c), _edge(w, a, d)]]
            elif len(ins) == 2:
                (a, b), (c, d) = ins, out
                tris = [[_edge(w, a, c), _edge(w, a, d), _edge(w, b, d)], [_edge(w, a, c), _edge(w, b, d), _edge(w, b, c)]]
            if tris:
                towards = OFFSETS[[w[n] for n in out]].mean(0) - OFFSETS[[w[n] for n in ins]].mean(0)
                for t in tris:
                    q = [_midpoint(v) for v in t]
                    s = float(np.cross(q[1] - q[0], q[2] - q[0]) @ towards)
                    assert s != 0.0
                    if s < 0:
                        t[1], t[2] = t[2], t[1]
            row.append([tuple(t) for t in tris])
        table.append(row)
    return table


def pack_case(tris):
    """One table entry as the kernel holds it: bits 0..1 the number of triangles, then 6 bits per vertex
    (owner corner << 3 | edge type), triangle 0 first."""
    word = len(tris)
    for i, v in enumerate(v for t in tris for v in t):
        word |= (v[0] << 3 | v[1]) << (2 + 6 * i)
    return word


def print_case_table():
    """The constexpr table of csrc/lfgc_mesh.hip."""
    lines = []
    for k, row in enumerate(case_table()):
        lines.append('    ' + ', '.join('0x%010xull' % pack_case(t) for t in row) + ',    // tetrahedron %d: %s' % (k, PERMS[k]))
    return '\n'.join(lines)


CASES = case_table()


# ---- one slab: the contract of lfgc_iso_mesh_count_f32 / lfgc_iso_mesh_emit_f32 ---------------------------------------------

def edge_flags(values, iso):
    """(nx, ny, nz, 7) bool: edge (p, ty) exists inside these planes and inside() differs at its ends; [..., ty - 1]."""
    ins = IR.inside(values, iso)
    nx, ny, nz = ins.shape
    fl = np.zeros((nx, ny, nz, 7), bool)
    for ty in range(1, 8):
        ox, oy, oz = OFFSETS[ty]
        fl[:nx - ox, :ny - oy, :nz - oz, ty - 1] = ins[:nx - ox, :ny - oy, :nz - oz] != ins[ox:, oy:, oz:]
    return fl


def _cell_masks(values, iso, n_cell_planes):
    """(n_cell_planes, ny-1, nz-1) 8-bit inside masks of the cells, bit c = inside(corner c)."""
    ins = IR.inside(values, iso)
    nx, ny, nz = ins.shape
    cm = np.zeros((n_cell_planes, ny - 1, nz - 1), np.int64)
    for c in range(8):
        ox, oy, oz = OFFSETS[c]
        cm |= ins[ox:ox + n_cell_planes, oy:oy + ny - 1, oz:oz + nz - 1].astype(np.int64) << c
    return cm


def _tet_masks(cm):
    out = []
    for k in range(6):
        w = tet_corners(k)
        out.append(sum(((cm >> w[n]) & 1) << n for n in range(4)))
    return out


def slab_planes(nx, n_owner):
    """(planes whose flags are ranked, planes of cells) of a slab of nx planes with n_owner owner planes."""
    return min(n_owner + 1, nx), min(n_owner, nx - 1)


def count(values, n_owner, iso):
    """(vertices owned by the first n_owner planes, triangles of the cells below them)."""
    values = np.asarray(values, F)
    nf, nc = slab_planes(values.shape[0], n_owner)
    fl = edge_flags(values, iso)
    ntri = np.array([len(t) for row in CASES for t in row]).reshape(6, 16)
    T = 0
    if nc > 0:
        for k, m in enumerate(_tet_masks(_cell_masks(values, iso, nc))):
            T += int(ntri[k][m].sum())
    return int(fl[:n_owner].sum()), T


def emit(values, n_owner, iso, xs, ys, zs, vertex_base):
    """(origins (n,3), dirs (n,3), bracket (n,4), triangles (T,3) int32) of one slab; xs holds the slab's planes."""
    values = np.asarray(values, F)
    xs, ys, zs = (np.asarray(a, F) for a in (xs, ys, zs))
    nx, ny, nz = values.shape
    nf, nc = slab_planes(nx, n_owner)
    fl = edge_flags(values, iso)[:nf]
    rank = (np.cumsum(fl.reshape(-1)) - fl.reshape(-1)).reshape(fl.shape)          # exclusive, order (x, y, z, ty)
    x, y, z, e = np.nonzero(fl[:n_owner])
    o = OFFSETS[e + 1]
    origins = np.stack([xs[x], ys[y], zs[z]], 1).astype(F)
    ends = np.stack([xs[x + o[:, 0]], ys[y + o[:, 1]], zs[z + o[:, 2]]], 1).astype(F)
    dirs = (ends - origins).astype(F)
    iso = F(iso)
    with np.errstate(invalid='ignore'):
        f_lo = (values[x, y, z] - iso).astype(F)
        f_hi = (values[x + o[:, 0], y + o[:, 1], z + o[:, 2]] - iso).astype(F)
    bracket = np.stack([np.zeros(len(x), F), np.ones(len(x), F), f_lo, f_hi], 1).astype(F)
    rows = []
    if nc > 0:
        cm = _cell_masks(values, iso, nc)
        cx, cy, cz = np.meshgrid(np.arange(nc), np.arange(ny - 1), np.arange(nz - 1), indexing='ij')
        lin = (cx * (ny - 1) + cy) * (nz - 1) + cz
        for k, mk in enumerate(_tet_masks(cm)):
            for m in range(1, 15):
                sel = mk == m
                if not sel.any():
                    continue
                for j, tri in enumerate(CASES[k][m]):
                    ids = []
                    for (c, ty) in tri:
                        oc = OFFSETS[c]
                        ids.append(rank[cx[sel] + oc[0], cy[sel] + oc[1], cz[sel] + oc[2], ty - 1] + int(vertex_base))
                    rows.append(np.stack([lin[sel], np.full(sel.sum(), k), np.full(sel.sum(), j)] + ids, 1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
        tris = rows[:, 3:].astype(np.int32)
    else:
        tris = np.zeros((0, 3), np.int32)
    return origins, dirs, bracket, tris


# ---- the loop of Mesh.isosurface_mesh ---------------------------------------------------------------------------------------

def slabs(X, owner_planes):
    """[(x0, x1, xe)]: owner planes [x0, x1), planes given [x0, xe) with xe = min(x1 + 2, X).  owner_planes None: one slab."""
    if owner_planes is None or owner_planes + 2 >= X:
        return [(0, X, X)]
    out, x0 = [], 0
    while x0 < X:
        if X - x0 <= owner_planes + 2:
            out.append((x0, X, X))
            break
        out.append((x0, x0 + owner_planes, x0 + owner_planes + 2))
        x0 += owner_planes
    return out


def mesh(lattice_values, xs, ys, zs, iso, refine_steps=0, value_of=None, owner_planes=None):
    """The whole loop on the lattice values (X, Y, Z): per slab count, emit, ``refine_steps`` bisections with
    ``value_of(positions (n, 3) float32) -> n values``, the secant step.  Returns a dict: vertices (V,3), triangles (T,3)
    int32, origins, dirs, bracket (the final brackets) and, with value_of, values (V,)."""
    lattice_values = np.asarray(lattice_values, F)
    X = lattice_values.shape[0]
    xs = np.asarray(xs, F)
    parts = dict(vertices=[], triangles=[], origins=[], dirs=[], bracket=[])
    nv = 0
    for x0, x1, xe in slabs(X, owner_planes):
        vals = lattice_values[x0:xe]
        V, T = count(vals, x1 - x0, iso)
        o, d, br, tr = emit(vals, x1 - x0, iso, xs[x0:xe], ys, zs, nv)
        assert len(o) == V and len(tr) == T
        rays = np.arange(V)
        v = None
        for _ in range(refine_steps):
            br, pos = IR.refine(rays, v, o, d, iso, br)
            v = np.asarray(value_of(pos), F)
        if v is not None:
            br, _ = IR.refine(rays, v, o, d, iso, br)
        _, p = IR.finish(rays, o, d, br) if V else (None, np.zeros((0, 3), F))
        for k, a in (('vertices', p), ('triangles', tr), ('origins', o), ('dirs', d), ('bracket', br)):
            parts[k].append(a)
        nv += V
    out = {k: np.concatenate(v) for k, v in parts.items()}
    if value_of is not None:
        out['values'] = np.asarray(value_of(out['vertices']), F) if len(out['vertices']) else np.zeros(0, F)
    return out


# ---- topology and measures -------------------------------------------------------------------------------------------------

def directed_edges(tris):
    """{(a, b): number of triangles that run a -> b}."""
    t = np.asarray(tris, np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    u, c = np.unique(e, axis=0, return_counts=True)
    return {(int(a), int(b)): int(n) for (a, b), n in zip(u, c)}


def undirected_edges(tris):
    """{(a, b) with a < b: number of triangles on the edge}."""
    out = {}
    for (a, b), n in directed_edges(tris).items():
        key = (min(a, b), max(a, b))
        out[key] = out.get(key, 0) + n
    return out


def is_closed(tris):
    return all(n == 2 for n in undirected_edges(tris).values())


def is_oriented(tris):
    """No directed edge twice: neighbouring triangles run along their shared edge in opposite directions."""
    return all(n == 1 for n in directed_edges(tris).values())


def euler_characteristic(n_vertices, tris):
    return int(n_vertices) - len(undirected_edges(tris)) + len(tris)


def triangle_normals(vertices, tris):
    """(T, 3) float64 (q1 - q0) x (q2 - q0): twice the area, pointing out of {v >= iso}."""
    q = np.asarray(vertices, np.float64)[np.asarray(tris, np.int64)]
    return np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])


def area(vertices, tris):
    return 0.5 * float(np.linalg.norm(triangle_normals(vertices, tris), axis=1).sum())


# ---- shared inputs ------------------------------------------------------------------------------------------------------------

def lattice(shape, lo=-1.0, hi=1.0):
    """(xs, ys, zs) float32 linspace tables and the (X, Y, Z, 3) float64 positions of their float32 values."""
    tabs = [np.linspace(lo, hi, n).astype(F) for n in shape]
    P = np.stack(np.meshgrid(*[t.astype(np.float64) for t in tabs], indexing='ij'), -1)
    return tabs, P


SPHERE_C, SPHERE_R = np.array([0.05, -0.03, 0.02]), 0.7


def sphere_field(P):
    return (SPHERE_R - np.linalg.norm(P - SPHERE_C, axis=-1)).astype(F)


def torus_field(P, R=0.55, r=0.25):
    """Axis z through (0.02, -0.01, 0.03)."""
    q = P - np.array([0.02, -0.01, 0.03])
    return (r - np.sqrt((np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - R) ** 2 + q[..., 2] ** 2)).astype(F)


def two_spheres_field(P):
    a = 0.3 - np.linalg.norm(P - np.array([-0.5, 0.02, 0.01]), axis=-1)
    b = 0.3 - np.linalg.norm(P - np.array([0.5, -0.02, 0.03]), axis=-1)
    return np.maximum(a, b).astype(F)


def random_case(shape, seed, iso=0.25):
    """Random lattice values with planted NaNs and values == iso, and irregular ascending axis tables."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, shape).astype(F)
    n = v.size
    flat = v.reshape(-1)
    flat[rng.choice(n, max(1, n // 23), replace=False)] = F(iso)
    flat[rng.choice(n, max(1, n // 37), replace=False)] = np.nan
    tabs = [np.cumsum(rng.uniform(0.01, 0.2, s)).astype(F) - F(1) for s in shape]
    return v, tabs, iso


GPU_LATTICES = ((2, 2, 2), (5, 6, 7), (33, 9, 34), (3, 3, 130), (2, 5, 3),
                (3, 300, 300))                     # 132 block counts: the scan of them (csrc/lfgc_select.hip) passes one wave
CARRY_LATTICE = (5, 520, 1030)                     # 1308 block counts per array: past one round of 1024 of that scan


# ---- the network case of the GPU test (conditions checked on the CPU in test_mesh_host.py) -----------------------------------

NET_SHAPE, NET_SEED = (5, 8, 20, 2), 9301          # the smallest build_synth model of the ray caster's test
NET_RES = (24, 20, 17)
NET_ISO = -0.33734                                 # the middle of a 2.8e-4 wide gap of the oracle's 8160 lattice values (-0.58 .. -0.14)
NET_NEAR = 1e-4                                     # no oracle lattice value within this of iso; the forward's parity bound is 2e-5
NET_REFINE = 6


def net_lattice_tables(res=NET_RES):
    """(dataset, axis tables, positions (X, Y, Z, 3)) of the (24, 20, 17) lattice as IndexDataset.tile_positions forms them
    in float32: the volume is one 32-voxel tile, so these are the positions of the fused forward's lattice mode."""
    from latent_feature_grid_compression_amd.data.IndexDataset import IndexDataset
    ds = IndexDataset(res, build_index_table=False)
    pos = ds.tile_positions((0, 0, 0), res).numpy()
    return ds, [pos[:, 0, 0, 0].copy(), pos[0, :, 0, 1].copy(), pos[0, 0, :, 2].copy()], pos


_ORACLE = {}


def oracle_net():
    """``value_of(positions, gradient=False)`` of the oracle's network with the parameters of build_synth(*NET_SHAPE,
    seed=NET_SEED): float32 values clamped to [-1, 1] like the eval-mode output, and with gradient=True also the autograd
    gradient of the unclamped output (n, 3).  Computed once per process and shared."""
    if 'fn' not in _ORACLE:
        import torch
        from oracle import ref_torch as R
        C, G, H, L = NET_SHAPE
        sm = R.synth_model(C, G, H, L, seed=NET_SEED)
        dense = R.decode_volume(sm['coeffs'], sm['shape_array'], sm['filter_rev'])

        def value_of(pos, gradient=False):
            p = torch.from_numpy(np.ascontiguousarray(pos, F).reshape(-1, 3)).clone().requires_grad_(gradient)
            with torch.enable_grad() if gradient else torch.no_grad():
                y = R.forward_from_grid(dense, sm['weights'], sm['biases'], p, 2).squeeze(-1)
                if gradient:
                    y.sum().backward()
            v = np.clip(y.detach().numpy().astype(F), F(-1), F(1))
            return (v, p.grad.numpy()) if gradient else v
        _ORACLE['fn'] = value_of
    return _ORACLE['fn']


def oracle_net_case():
    """The network case by the oracle alone, computed once: lattice values, the meshes at refine_steps 0 and NET_REFINE."""
    if 'case' not in _ORACLE:
        value_of = oracle_net()
        ds, tabs, pos = net_lattice_tables()
        lat = value_of(pos.reshape(-1, 3)).reshape(NET_RES)
        m0 = mesh(lat, *tabs, NET_ISO, 0, value_of)
        m6 = mesh(lat, *tabs, NET_ISO, NET_REFINE, value_of)
        _ORACLE['case'] = dict(dataset=ds, tables=tabs, lattice=lat, coarse=m0, fine=m6)
    return _ORACLE['case']


def winding_agreement(vertices, tris, normals):
    """(share of the vertex-triangle incidences with normal . triangle normal > 0, their number)."""
    tn = triangle_normals(vertices, tris)
    dots = (np.asarray(normals, np.float64)[np.asarray(tris, np.int64)] * tn[:, None, :]).sum(-1)
    return float((dots > 0).mean()), dots.size
