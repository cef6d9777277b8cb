// lfgc_mesh.hip -- isosurface triangle meshes of a lattice of values (gfx950): marching tetrahedra on the Kuhn triangulation
// of the volume lattice, one x-slab at a time.  The values come from lfgc_forward_f32 in lattice mode, the
// vertex positions from lfgc_ray_iso_refine_f32 / lfgc_ray_iso_finish_f32 on the brackets emitted here; what this file adds
// is the classification, the stream compaction and the connectivity between them.
//   lfgc_iso_mesh_count_f32  classify every lattice point (7-bit crossing-edge flag) and every cell (0..12 triangles), exclusive
//                            prefix sums of both with the block sum and the scan of lfgc_select.h, the two totals
//   lfgc_iso_mesh_emit_f32   per owned crossing edge its origin, direction and bracket; per triangle three vertex indices
// A thread owns one lattice point (and the cell whose lowest corner it is); consecutive lanes walk z, the contiguous axis, so
// the eight corner loads of a wave are eight contiguous rows.  No atomics: every output address has one writer.
#include "lfgc_ray.h"
#include "lfgc_select.h"

namespace {

constexpr int kBlock = kSelectBlock;            // the classify pass ends in lfgc_select_block_sum
constexpr int kItems = 8;                       // lattice points per thread in the count and prefix passes
constexpr int kPerBlock = kBlock * kItems;
constexpr long long kMaxPoints = 1ll << 27;     // 12 triangles and 7 vertices per point stay below 2^31 in a slab

// Tetrahedron k = permutation k of (0,1,2) in lexicographic order; its corners as cube corner codes (x << 2 | y << 1 | z):
// w0 = 0, w1 = kW1[k], w2 = kW2[k], w3 = 7.
constexpr int kW1[6] = {4, 4, 2, 2, 1, 1};
constexpr int kW2[6] = {6, 5, 6, 3, 5, 3};

// kCase[k * 16 + m]: the triangles of tetrahedron k with inside mask m (bit n = inside(w_n)).  Bits 0..1: their number; then
// 6 bits per vertex, triangle 0 first: owner cube corner << 3 | edge type.  Printed by tests/mesh_ref.py (print_case_table),
// which generates it from the geometric rule; tests/test_mesh_host.py compares this text with that output.
__constant__ unsigned long long kCase[96] = {
    0x0000000000ull, 0x000001c611ull, 0x000008a311ull, 0x228c68c71aull, 0x00000c6219ull, 0x318841f112ull, 0x06c44c6312ull, 0x00000c631dull, 0x000008f11dull, 0x23c44c4612ull, 0x311c48b112ull, 0x000008b119ull, 0x078c68e21aull, 0x000008e211ull, 0x0000018711ull, 0x0000000000ull,    // tetrahedron 0: (0, 1, 2)
    0x0000000000ull, 0x0000014711ull, 0x000008e111ull, 0x238451e316ull, 0x0000086a15ull, 0x21a84a8712ull, 0x2a1448ea12ull, 0x000008ea1dull, 0x00000aa31dull, 0x2a8c416a12ull, 0x07a84aa112ull, 0x00000aa115ull, 0x231c586316ull, 0x0000086311ull, 0x000001c511ull, 0x0000000000ull,    // tetrahedron 1: (0, 2, 1)
    0x0000000000ull, 0x0000018709ull, 0x0000055409ull, 0x155061d51aull, 0x0000053119ull, 0x14c42c470aull, 0x311825710aull, 0x000005711dull, 0x00000c551dull, 0x315421b10aull, 0x07c42c540aull, 0x00000c5419ull, 0x151c65151aull, 0x0000051509ull, 0x000001c609ull, 0x0000000000ull,    // tetrahedron 2: (1, 0, 2)
    0x0000000000ull, 0x000001c309ull, 0x0000045509ull, 0x115435470eull, 0x000007110dull, 0x1c4421dc0aull, 0x037027150aull, 0x000007151dull, 0x0000055c1dull, 0x157027030aull, 0x1c1c245c0aull, 0x0000045c0dull, 0x075435510eull, 0x0000055109ull, 0x000000c709ull, 0x0000000000ull,    // tetrahedron 3: (1, 2, 0)
    0x0000000000ull, 0x000001c505ull, 0x0000030e05ull, 0x0c38538716ull, 0x00000a8c15ull, 0x2a3011ea06ull, 0x05a81a8e06ull, 0x00000a8e1dull, 0x000003aa1dull, 0x0ea81a8506ull, 0x2a1c132a06ull, 0x0000032a15ull, 0x0738538c16ull, 0x0000038c05ull, 0x0000014705ull, 0x0000000000ull,    // tetrahedron 4: (2, 0, 1)
    0x0000000000ull, 0x000000c705ull, 0x0000038a05ull, 0x0e2831ce0eull, 0x0000029c0dull, 0x0a70170706ull, 0x1c0c139c06ull, 0x0000039c1dull, 0x0000070e1dull, 0x1c3810dc06ull, 0x0770170a06ull, 0x0000070a0dull, 0x0e1c328e0eull, 0x0000028e05ull, 0x000001c305ull, 0x0000000000ull,    // tetrahedron 5: (2, 1, 0)
};

// A slab of nx planes of which the first n_owner own their edges.  Edges are ranked for the planes [0, nf): the owner planes
// and the one after them, which the last cells reference.  Cells exist in the planes [0, nc).
struct Slab {
    int nx, ny, nz, nf, nc;
    unsigned plane;              // ny * nz
    unsigned npts;               // nf * plane: the points that are classified
    unsigned v_split;            // n_owner * plane clipped to npts: the points before it own this slab's vertices
    float iso;
};

struct Workspace {
    long long* offsets;          // [2][nblocks]: exclusive block offsets of the vertex and the triangle counts
    int* vpre;                   // [npts padded]: exclusive vertex prefix of every point
    int* tpre;                   // [npts padded]: exclusive triangle prefix of every cell (indexed by its lowest corner)
    unsigned* block_counts;      // [2][nblocks]
    unsigned short* codes;       // [npts padded]: crossing-edge flag (bits 0..6, bit ty-1) | triangle count << 8
};

inline long long blocks_of(long long npts) { return (npts + kPerBlock - 1) / kPerBlock; }

inline long long align16(long long b) { return (b + 15) & ~15ll; }

inline long long carve(void* base, long long npts, Workspace* w) {
    const long long nb = blocks_of(npts), padded = nb * kPerBlock;
    char* p = static_cast<char*>(base);
    long long at = 0;
    if (w) w->offsets = reinterpret_cast<long long*>(p + at);
    at += align16(2 * nb * 8);
    if (w) w->vpre = reinterpret_cast<int*>(p + at);
    at += padded * 4;
    if (w) w->tpre = reinterpret_cast<int*>(p + at);
    at += padded * 4;
    if (w) w->block_counts = reinterpret_cast<unsigned*>(p + at);
    at += align16(2 * nb * 4);
    if (w) w->codes = reinterpret_cast<unsigned short*>(p + at);
    at += padded * 2;
    return at;
}

__device__ __forceinline__ void point_of(const Slab& s, unsigned i, int& lx, int& y, int& z) {
    lx = (int)(i / s.plane);
    const unsigned r = i - (unsigned)lx * s.plane;
    y = (int)(r / (unsigned)s.nz);
    z = (int)(r - (unsigned)y * (unsigned)s.nz);
}

__device__ __forceinline__ unsigned corner_offset(const Slab& s, int c) {
    return (unsigned)((c >> 2) & 1) * s.plane + (unsigned)((c >> 1) & 1) * (unsigned)s.nz + (unsigned)(c & 1);
}

// inside bits of the 8 corners of the cell at point i (bit c; corners outside the slab read as the point itself)
__device__ __forceinline__ unsigned corner_bits(const Slab& s, const float* __restrict__ values, unsigned i, unsigned exist) {
    const unsigned in0 = lfgc_iso_inside(values[i], s.iso) ? 1u : 0u;
    unsigned cm = in0;
#pragma unroll
    for (int c = 1; c < 8; ++c) {
        unsigned in = in0;
        if (exist >> c & 1) in = lfgc_iso_inside(values[i + corner_offset(s, c)], s.iso) ? 1u : 0u;
        cm |= in << c;
    }
    return cm;
}

__device__ __forceinline__ unsigned tet_mask(unsigned cm, int k) {
    return (cm & 1u) | ((cm >> kW1[k] & 1u) << 1) | ((cm >> kW2[k] & 1u) << 2) | ((cm >> 7 & 1u) << 3);
}

// flag | triangle count << 8 of point i
__device__ __forceinline__ unsigned classify(const Slab& s, const float* __restrict__ values, unsigned i) {
    int lx, y, z;
    point_of(s, i, lx, y, z);
    const unsigned ex = lx + 1 < s.nx ? 0xf0u : 0u, ey = y + 1 < s.ny ? 0xccu : 0u, ez = z + 1 < s.nz ? 0xaau : 0u;
    // corner c exists iff each of its set offset bits stays inside: x bit -> mask f0, y bit -> cc, z bit -> aa
    unsigned exist = 1u;
#pragma unroll
    for (int c = 1; c < 8; ++c) {
        const bool ok = (!(c & 4) || ex) && (!(c & 2) || ey) && (!(c & 1) || ez);
        exist |= ok ? 1u << c : 0u;
    }
    const unsigned cm = corner_bits(s, values, i, exist);
    const unsigned flag = ((cm ^ ((cm & 1u) ? 0xffu : 0u)) & exist) >> 1;          // bit ty-1: edge ty exists and crosses
    unsigned ntri = 0;
    if (exist == 0xffu && lx < s.nc) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int pc = __popc(tet_mask(cm, k));
            ntri += pc == 2 ? 2u : (pc == 1 || pc == 3 ? 1u : 0u);
        }
    }
    return flag | ntri << 8;
}

// pass 1: codes of all points, vertex and triangle counts per workgroup
__global__ __launch_bounds__(kBlock) void mesh_classify_kernel(const Slab s, const float* __restrict__ values, Workspace w,
                                                               unsigned nblocks) {
    const unsigned base = blockIdx.x * (unsigned)kPerBlock;
    unsigned c[2] = {0, 0};                                 // vertices, triangles
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const unsigned i = base + j * kBlock + threadIdx.x;
        unsigned code = 0;
        if (i < s.npts) code = classify(s, values, i);
        w.codes[i] = (unsigned short)code;                  // the padded tail is zeroed: the prefix pass reads whole chunks
        c[0] += __popc(code & 0x7fu);
        c[1] += code >> 8;
    }
    lfgc_select_block_sum(c);
    if (threadIdx.x == 0) {
        w.block_counts[blockIdx.x] = c[0];
        w.block_counts[nblocks + blockIdx.x] = c[1];
    }
}

// pass 2: lfgc_select_scan of the block counts, array 0 the vertices, array 1 the triangles.  totals[1] = all triangles;
// totals[0] = all vertices when every classified point is an owner (else pass 3 writes it).

// pass 3: exclusive prefix of every point.  A thread takes 8 consecutive points (one 16-byte load of codes, two 32-byte
// stores of prefixes); the thread sums are scanned across the workgroup.
__global__ __launch_bounds__(kBlock) void mesh_prefix_kernel(const Slab s, Workspace w, unsigned nblocks, long long* __restrict__ totals) {
    const unsigned i0 = blockIdx.x * (unsigned)kPerBlock + threadIdx.x * kItems;
    const uint4 raw = *reinterpret_cast<const uint4*>(w.codes + i0);
    const unsigned word[4] = {raw.x, raw.y, raw.z, raw.w};
    unsigned nv[kItems], nt[kItems];
    unsigned sumv = 0, sumt = 0;
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const unsigned code = (word[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
        nv[j] = __popc(code & 0x7fu);
        nt[j] = code >> 8;
        sumv += nv[j];
        sumt += nt[j];
    }
    unsigned iv = sumv, it = sumt;                      // inclusive across the wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned a = __shfl_up(iv, off), b = __shfl_up(it, off);
        if (lane >= off) { iv += a; it += b; }
    }
    __shared__ unsigned swv[4], swt[4];
    if (lane == 63) { swv[wave] = iv; swt[wave] = it; }
    __syncthreads();
    unsigned pv = iv - sumv, pt = it - sumt;
    for (int k = 0; k < wave; ++k) { pv += swv[k]; pt += swt[k]; }
    pv += (unsigned)w.offsets[blockIdx.x];
    pt += (unsigned)w.offsets[nblocks + blockIdx.x];
    int ov[kItems], ot[kItems];
#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        ov[j] = (int)pv;
        ot[j] = (int)pt;
        if (i0 + j == s.v_split) totals[0] = (long long)pv;          // at most one thread of the launch
        pv += nv[j];
        pt += nt[j];
    }
    int4* dv = reinterpret_cast<int4*>(w.vpre + i0);
    int4* dt = reinterpret_cast<int4*>(w.tpre + i0);
    dv[0] = make_int4(ov[0], ov[1], ov[2], ov[3]);
    dv[1] = make_int4(ov[4], ov[5], ov[6], ov[7]);
    dt[0] = make_int4(ot[0], ot[1], ot[2], ot[3]);
    dt[1] = make_int4(ot[4], ot[5], ot[6], ot[7]);
}

// thread = one owner point: its crossing edges in ascending type
__global__ __launch_bounds__(kBlock) void mesh_vertices_kernel(const Slab s, const float* __restrict__ values, const Workspace w,
                                                               const float* __restrict__ xs, const float* __restrict__ ys,
                                                               const float* __restrict__ zs, long long max_vertices,
                                                               float* __restrict__ origins, float* __restrict__ dirs,
                                                               float4* __restrict__ bracket) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (i >= s.v_split) return;
    const unsigned flag = w.codes[i] & 0x7fu;
    if (!flag) return;
    int lx, y, z;
    point_of(s, i, lx, y, z);
    const float px = xs[lx], py = ys[y], pz = zs[z];
    const float f0 = values[i] - s.iso;
    long long row = w.vpre[i];
#pragma unroll
    for (int ty = 1; ty < 8; ++ty) {
        if (!(flag >> (ty - 1) & 1)) continue;
        if (row < max_vertices) {
            // a flag bit says the far end exists inside the slab: the table reads below stay inside nx, ny, nz entries
            const float qx = (ty & 4) ? xs[lx + 1] : px, qy = (ty & 2) ? ys[y + 1] : py, qz = (ty & 1) ? zs[z + 1] : pz;
            origins[row * 3 + 0] = px; origins[row * 3 + 1] = py; origins[row * 3 + 2] = pz;
            dirs[row * 3 + 0] = qx - px; dirs[row * 3 + 1] = qy - py; dirs[row * 3 + 2] = qz - pz;
            bracket[row] = make_float4(0.0f, 1.0f, f0, values[i + corner_offset(s, ty)] - s.iso);
        }
        ++row;
    }
}

// thread = one cell (indexed by its lowest corner): its tetrahedra 0..5, their triangles in table order
__global__ __launch_bounds__(kBlock) void mesh_triangles_kernel(const Slab s, const float* __restrict__ values, const Workspace w,
                                                                long long vertex_base, long long max_triangles,
                                                                int* __restrict__ triangles) {
    const unsigned i = blockIdx.x * (unsigned)kBlock + threadIdx.x;
    if (i >= (unsigned)s.nc * s.plane) return;
    if (!(w.codes[i] >> 8)) return;                      // also every point that is not the lowest corner of a cell
    const unsigned cm = corner_bits(s, values, i, 0xffu);
    long long row = w.tpre[i];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned m = tet_mask(cm, k);
        if (m == 0u || m == 15u) continue;
        unsigned long long word = kCase[k * 16 + m];
        const int n = (int)(word & 3u);
        word >>= 2;
        for (int t = 0; t < n; ++t) {
            int id[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned v = (unsigned)(word & 63u);
                word >>= 6;
                const unsigned p = i + corner_offset(s, (int)(v >> 3));                // p < npts: the cell lies below plane nf
                const unsigned below = (1u << ((v & 7u) - 1u)) - 1u;
                id[q] = (int)(vertex_base + w.vpre[p] + __popc(w.codes[p] & 0x7fu & below));
            }
            if (row < max_triangles) {
                triangles[row * 3 + 0] = id[0]; triangles[row * 3 + 1] = id[1]; triangles[row * 3 + 2] = id[2];
            }
            ++row;
        }
    }
}

// LFGC_OK and the slab's plan, or the argument error
inline int make_slab(int nx, int n_owner, int ny, int nz, float iso, Slab* s) {
    if (nx < 1 || n_owner < 1 || n_owner > nx || ny < 2 || nz < 2 || !lfgc_finite(iso)) return LFGC_E_SHAPE;
    if ((long long)nx * ny * nz > kMaxPoints) return LFGC_E_UNSUPPORTED;
    s->nx = nx; s->ny = ny; s->nz = nz;
    s->nf = n_owner + 1 < nx ? n_owner + 1 : nx;
    s->nc = n_owner < nx - 1 ? n_owner : nx - 1;
    s->plane = (unsigned)ny * (unsigned)nz;
    s->npts = (unsigned)s->nf * s->plane;
    s->v_split = (unsigned)n_owner * s->plane;          // n_owner <= nf, so v_split <= npts
    s->iso = iso;
    return LFGC_OK;
}

}  // namespace

extern "C" int64_t lfgc_iso_mesh_workspace_bytes(int32_t nx, int32_t n_owner, int32_t ny, int32_t nz) {
    Slab s;
    if (make_slab(nx, n_owner, ny, nz, 0.0f, &s) != LFGC_OK) return 16;
    return carve(nullptr, s.npts, nullptr);
}

extern "C" int lfgc_iso_mesh_count_f32(const float* values, int32_t nx, int32_t n_owner, int32_t ny, int32_t nz, float iso,
                                       int64_t* totals, void* workspace, int64_t workspace_bytes, lfgc_stream_t stream) {
    if (!values || !totals || !workspace) return LFGC_E_NULL;
    Slab s;
    const int err = make_slab(nx, n_owner, ny, nz, iso, &s);
    if (err != LFGC_OK) return err;
    if ((uintptr_t)workspace & 15) return LFGC_E_ALIGN;
    if (workspace_bytes < carve(nullptr, s.npts, nullptr)) return LFGC_E_WORKSPACE;
    Workspace w;
    carve(workspace, s.npts, &w);
    const long long nb = blocks_of(s.npts);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_classify_kernel, dim3((unsigned)nb), dim3(kBlock), 0, st, s, values, w, (unsigned)nb);
    LFGC_HIP_CHECK_LAUNCH();
    long long* tot = reinterpret_cast<long long*>(totals);
    const int rc = lfgc_select_scan(w.block_counts, w.offsets, nb, 2, LfgcScanTotals{{s.v_split == s.npts ? tot : nullptr, tot + 1}}, st);
    if (rc != LFGC_OK) return rc;
    hipLaunchKernelGGL(mesh_prefix_kernel, dim3((unsigned)nb), dim3(kBlock), 0, st, s, w, (unsigned)nb, reinterpret_cast<long long*>(totals));
    LFGC_HIP_CHECK_LAUNCH();
    return LFGC_OK;
}

extern "C" int lfgc_iso_mesh_emit_f32(const float* values, int32_t nx, int32_t n_owner, int32_t ny, int32_t nz, float iso,
                                      const float* xs, const float* ys, const float* zs, int64_t vertex_base,
                                      const void* workspace, int64_t workspace_bytes, int64_t n_vertices, int64_t n_triangles,
                                      float* origins, float* dirs, float* bracket, int32_t* triangles, lfgc_stream_t stream) {
    if (n_vertices == 0 && n_triangles == 0) return LFGC_OK;
    if (!values || !xs || !ys || !zs || !workspace) return LFGC_E_NULL;
    if (n_vertices > 0 && (!origins || !dirs || !bracket)) return LFGC_E_NULL;
    if (n_triangles > 0 && !triangles) return LFGC_E_NULL;
    Slab s;
    const int err = make_slab(nx, n_owner, ny, nz, iso, &s);
    if (err != LFGC_OK) return err;
    if (n_vertices < 0 || n_triangles < 0 || vertex_base < 0 || vertex_base > 0x7fffffffLL) return LFGC_E_SHAPE;
    if (((uintptr_t)workspace | (uintptr_t)bracket) & 15) return LFGC_E_ALIGN;
    if (workspace_bytes < carve(nullptr, s.npts, nullptr)) return LFGC_E_WORKSPACE;
    Workspace w;
    carve(const_cast<void*>(workspace), s.npts, &w);
    hipStream_t st = (hipStream_t)stream;
    if (n_vertices > 0) {
        hipLaunchKernelGGL(mesh_vertices_kernel, dim3((s.v_split + kBlock - 1) / kBlock), dim3(kBlock), 0, st, s, values, w, xs, ys, zs,
                           (long long)n_vertices, origins, dirs, reinterpret_cast<float4*>(bracket));
        LFGC_HIP_CHECK_LAUNCH();
    }
    const unsigned ncells = (unsigned)s.nc * s.plane;
    if (n_triangles > 0 && ncells > 0) {
        hipLaunchKernelGGL(mesh_triangles_kernel, dim3((ncells + kBlock - 1) / kBlock), dim3(kBlock), 0, st, s, values, w,
                           (long long)vertex_base, (long long)n_triangles, triangles);
        LFGC_HIP_CHECK_LAUNCH();
    }
    return LFGC_OK;
}
