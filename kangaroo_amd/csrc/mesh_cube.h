// mesh_cube.h -- marching cubes over a CUBE SOURCE: everything the dense volume's extractor (mesh.hip: kfx_mc_*, kfx_mesh_*,
// kfx_mesh_index_*) and the packed bricks' (mesh_bricks.hip: kfx_mesh_bricks_*) do alike, written once, so that a brick mesh is the
// dense mesh of the volume its bricks unpack into, and a brick index the weld of that soup, because one text computes both:
//   * the case tables in __constant__ memory and their loader (every translation unit has its own device symbols, see below);
//   * a cube's corners' case, a vertex's position on its edge, its store;
//   * the kernels that run one thread per ACTIVE cube -- k_mc_emit (the soup), k_mesh_own (which edges a cube owns) and
//     k_mc_emit_indexed (the weld), the last two over the ActiveCube prologue -- as templates over the source, instantiated by each file;
//   * of the indexed extractions how a lattice edge is named in its owner, how a cube ranks the edges it owns, k_mesh_vertex_base;
//   * of the two-step calls the block sums, their scan kernel, the scratch carver and the read-back of a plan's totals.
// What a source answers -- where a listed cube is, its corner values, a vertex's normal and grey, the triangle slots it may write,
// the owner of a lattice edge -- is stated above k_mc_emit; DenseCubes (mesh.hip: pitched rows, slabs) and BrickCubes
// (mesh_bricks.hip: bricks through a neighbour table) are the two.  The plan passes (counting and compaction) differ in substance
// and stay each file's.
#pragma once

#include "kfx_device.h"
#include "sampling.h"
#include "host_args.h"
#include "block_scan.h"

namespace kfx {

// The case tables (mc_tables.inc) in __constant__ memory.  A device symbol belongs to one code object, so each translation unit that
// includes this has, and loads, its own -- in a namespace it names with KFX_MESH_UNIT before the include, so that the host's shadows
// of the two do not clash.  (Not static: a static __constant__ that the host names is reached through the GOT, one more dependent
// scalar load per table in every kernel; profiles/mesh_shared/codegen.txt.)
#ifndef KFX_MESH_UNIT
#error "define KFX_MESH_UNIT, this translation unit's name for its case tables, before including mesh_cube.h"
#endif
#include "mc_tables.inc"
namespace KFX_MESH_UNIT {
__constant__ unsigned char c_num_tris[256];
__constant__ unsigned short c_edge_mask[256];
__constant__ signed char c_tris[256][15];
}
using namespace KFX_MESH_UNIT;
static bool g_tables_loaded[64] = {};

static int load_tables()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (g_tables_loaded[dev]) return 0;
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_num_tris), MC_NUM_TRIS, sizeof(MC_NUM_TRIS));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_edge_mask), MC_EDGE_MASK, sizeof(MC_EDGE_MASK));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_tris), MC_TRIS, sizeof(MC_TRIS));
    if (e != hipSuccess) return set_error((int)e, hipGetErrorString(e));
    g_tables_loaded[dev] = true;
    return 0;
}

struct MeshParams {
    VolView vol;
    V3 size, dims1, hi2, voxel;  // members trilinear<>() / gradient<>() expect
    V3 inv_size;
    int fastdiv, off32;
    int cx, cy, cz;              // cubes per axis = dims - 1
    int avail_lo, avail_hi;      // planes that may be read: [0, d) of a whole volume, the stored planes of a slab
};

// corner i of the cube at (x, y, z): offsets (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1)
__device__ __forceinline__ int corner_dx(int i) { return ((i + 1) >> 1) & 1; }
__device__ __forceinline__ int corner_dy(int i) { return (i >> 1) & 1; }
__device__ __forceinline__ int corner_dz(int i) { return i >> 2; }

// the case index of 8 corner values; false if a corner is not finite (MarchingCubes.h:58-74)
__device__ __forceinline__ bool corner_case(const float v[8], int& flag)
{
    bool finite = true;
    int bits = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        finite = finite && isfinite(v[i]);
        if (v[i] <= 0.0f) bits |= 1 << i;
    }
    flag = bits;
    return finite;
}

// VoxelPositionInUnits(x,y,z) (BoundedVolume.h:115-125): the cube's corner 0
__device__ __forceinline__ V3 cube_origin(const MeshParams& p, int x, int y, int z)
{
    return v3(p.vol.bmin.x + p.size.x * (float)x / p.dims1.x, p.vol.bmin.y + p.size.y * (float)y / p.dims1.y,
              p.vol.bmin.z + p.size.z * (float)z / p.dims1.z);
}

// edges 0-3: bottom ring, 4-7: top ring, 8-11: verticals (MarchingCubes tables' numbering); the corners edge e joins
__device__ __forceinline__ constexpr int edge_c0(int e) { return e < 8 ? e : e - 8; }
__device__ __forceinline__ constexpr int edge_c1(int e) { return e < 4 ? (e + 1) & 3 : (e < 8 ? 4 + ((e + 1) & 3) : e - 4); }

// the vertex of the cube at p0 (corner values v) on its edge e; VoxelSizeUnits() (BoundedVolume.h:67-76) in p.voxel
__device__ __forceinline__ V3 edge_position(const MeshParams& p, const V3& p0, const float v[8], int e)
{
    const int c0 = edge_c0(e), c1 = edge_c1(e);
    // fGetOffset (MarchingCubes.h:25-32): the difference is a float, the quotient a double
    const double delta = (double)(v[c1] - v[c0]);
    const float off = delta == 0.0 ? 0.5f : (float)((double)(0.0f - v[c0]) / delta);
    const float ox = (float)corner_dx(c0), oy = (float)corner_dy(c0), oz = (float)corner_dz(c0);
    const float dx = (float)(corner_dx(c1) - corner_dx(c0)), dy = (float)(corner_dy(c1) - corner_dy(c0)),
                dz = (float)(corner_dz(c1) - corner_dz(c0));
    return v3(p0.x + (ox + off * dx) * p.voxel.x, p0.y + (oy + off * dy) * p.voxel.y, p0.z + (oz + off * dz) * p.voxel.z);
}

__device__ __forceinline__ void cube_xyz(const MeshParams& p, long long ci, int& x, int& y, int& z)
{
    z = (int)(ci % p.cz);
    y = (int)((ci / p.cz) % p.cy);
    x = (int)(ci / ((long long)p.cz * p.cy));
}

// vertex i of the output: position, normal and, with a colour volume, the grey C as ConvertPixel<float3,float>(c) = (c,c,c) in
// aiColor4D(c, c, c, 1)
__device__ __forceinline__ void store_vertex(float* verts, float* norms, float* colors, size_t i,
                                             const V3& P, const V3& N, float C, int has_color)
{
    verts[i * 3 + 0] = P.x; verts[i * 3 + 1] = P.y; verts[i * 3 + 2] = P.z;
    norms[i * 3 + 0] = N.x; norms[i * 3 + 1] = N.y; norms[i * 3 + 2] = N.z;
    if (has_color) {
        colors[i * 4 + 0] = C; colors[i * 4 + 1] = C; colors[i * 4 + 2] = C; colors[i * 4 + 3] = 1.0f;
    }
}

constexpr int MESH_SCAN_THREADS = 1024, MESH_SCAN_PER_THREAD = 8;
constexpr unsigned long long MESH_MAX_TRIS = 4294967296ull / 3;   // 2^32 / 3: vertex offsets stay 32-bit
constexpr size_t MESH_HEADER = 256;

// the sums of a pair of counters over a workgroup of 256 threads, one value of each per thread: part[2 b] = sum of a,
// part[2 b + 1] = sum of t for workgroup b (written by its thread 0)
__device__ __forceinline__ void store_block_sums(unsigned a, unsigned t, unsigned* __restrict__ part)
{
    __shared__ unsigned lds[2][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        t += __shfl_xor(t, o, 64);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { lds[0][wv] = a; lds[1][wv] = t; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = lds[0][0] + lds[0][1] + lds[0][2] + lds[0][3];
        part[2 * (size_t)blockIdx.x + 1] = lds[1][0] + lds[1][1] + lds[1][2] + lds[1][3];
    }
}

// one workgroup: exclusive 64-bit offsets of the blocks (base[2 b] cubes or vertices, base[2 b + 1] triangles) and the totals
static __global__ __launch_bounds__(MESH_SCAN_THREADS) void k_mesh_scan_partials(const unsigned* __restrict__ part, const long long nblk,
                                                                                 unsigned long long* __restrict__ base,
                                                                                 unsigned long long* __restrict__ totals)
{
    __shared__ unsigned long long lds[2][MESH_SCAN_THREADS / 64];
    unsigned long long run_a = 0, run_t = 0;
    constexpr int CHUNK = MESH_SCAN_THREADS * MESH_SCAN_PER_THREAD;
    for (long long c0 = 0; c0 < nblk; c0 += CHUNK) {
        const long long b0 = c0 + (long long)threadIdx.x * MESH_SCAN_PER_THREAD;
        unsigned va[MESH_SCAN_PER_THREAD], vt[MESH_SCAN_PER_THREAD];
        unsigned long long sa = 0, st = 0;
#pragma unroll
        for (int j = 0; j < MESH_SCAN_PER_THREAD; ++j) {
            const bool in = b0 + j < nblk;
            va[j] = in ? part[2 * (b0 + j)] : 0u;
            vt[j] = in ? part[2 * (b0 + j) + 1] : 0u;
            sa += va[j];
            st += vt[j];
        }
        unsigned long long ta, tt;
        unsigned long long ea = block_exclusive_scan<unsigned long long, MESH_SCAN_THREADS / 64>(sa, lds[0], &ta) + run_a;
        unsigned long long et = block_exclusive_scan<unsigned long long, MESH_SCAN_THREADS / 64>(st, lds[1], &tt) + run_t;
#pragma unroll
        for (int j = 0; j < MESH_SCAN_PER_THREAD; ++j) {
            if (b0 + j < nblk) {
                base[2 * (b0 + j)] = ea;
                base[2 * (b0 + j) + 1] = et;
            }
            ea += va[j];
            et += vt[j];
        }
        run_a += ta;
        run_t += tt;
    }
    if (threadIdx.x == 0) {
        totals[0] = run_a;
        totals[1] = run_t;
    }
}

// ---- what the indexed extractions share (mesh.hip: kfx_mesh_index_*; mesh_bricks.hip: kfx_mesh_bricks_index_*): a vertex is keyed by
// the LATTICE EDGE under its cube edge, and numbered by the cube that owns that edge.  Which cube owns it is each file's own rule (the
// first in ITS emission order); how an edge is named inside its owner and how a cube numbers the edges it owns is written here.
constexpr int MESH_IDX_BLOCK = 256;   // active cubes per scan block of an index plan

// The lattice edge under cube edge e: its axis a, the other two axes u < w (x before y before z), and m[3], the offsets of the edge's
// minimum corner from the cube's.  The four cubes around the edge sit at that minimum corner minus (su, sw) in {0, 1}^2 along u and w,
// i.e. at this cube plus (m[u] - su, m[w] - sw).
struct LatticeEdge {
    int m[3], a, u, w;
};
__device__ __forceinline__ LatticeEdge lattice_edge(int e)
{
    const int c0 = edge_c0(e), c1 = edge_c1(e);
    LatticeEdge l;
    l.m[0] = min(corner_dx(c0), corner_dx(c1));
    l.m[1] = min(corner_dy(c0), corner_dy(c1));
    l.m[2] = min(corner_dz(c0), corner_dz(c1));
    l.a = corner_dx(c0) != corner_dx(c1) ? 0 : (corner_dy(c0) != corner_dy(c1) ? 1 : 2);
    l.u = l.a == 0 ? 1 : 0;
    l.w = l.a == 2 ? 1 : 2;
    return l;
}
// the number, in the cube that sits at the edge's minimum corner minus (su, sw), of the edge of axis a
__device__ __forceinline__ int owner_e(int a, int su, int sw)
{
    return a == 0 ? 2 * su + 4 * sw : (a == 1 ? (su ? 1 : 3) + 4 * sw : 8 + (sw ? 3 - su : su));
}

// ranks of a cube's owned edges by first use in its triangle list (tris: the case's row of MC_TRIS, ntri triangles), 4 bits per edge
__device__ __forceinline__ unsigned long long edge_ranks(const signed char* tris, int ntri, unsigned own)
{
    unsigned long long ranks = 0;
    unsigned seen = 0, r = 0;
    const int n = ntri * 3;
    for (int k = 0; k < n; ++k) {
        const int q = tris[k];
        if ((seen >> q) & 1u) continue;
        seen |= 1u << q;
        if ((own >> q) & 1u) ranks |= (unsigned long long)(r++) << (4 * q);
    }
    return ranks;
}
__device__ __forceinline__ unsigned rank_of(unsigned long long ranks, int e) { return (unsigned)(ranks >> (4 * e)) & 15u; }

// every active cube's first vertex id: info[t] >> 8 is the mask of the edges cube t owns, base[2 b] the vertices before block b
static __global__ __launch_bounds__(MESH_IDX_BLOCK) void k_mesh_vertex_base(const unsigned* __restrict__ info, const long long n_active,
                                                                            const unsigned long long* __restrict__ base, unsigned* __restrict__ vbase)
{
    __shared__ unsigned lds[MESH_IDX_BLOCK / 64];
    const long long t = (long long)blockIdx.x * MESH_IDX_BLOCK + threadIdx.x;
    const unsigned n = t < n_active ? __popc(info[t] >> 8) : 0u;
    unsigned total;
    const unsigned ex = block_exclusive_scan<unsigned, MESH_IDX_BLOCK / 64>(n, lds, &total);
    if (t < n_active) vbase[t] = (unsigned)base[2 * (size_t)blockIdx.x] + ex;
}

// ---- the kernels with one thread per ACTIVE cube (cube_index lists the cubes with triangles in emission order, tri_offset their
// first triangle): dense lanes instead of the ~1 % active lanes of a thread-per-cube sweep.  They are written over a cube source SRC,
// a kernel argument that holds the geometry `p` (MeshParams) and answers, with a per-cube Home of its own (where the cube's cells are):
//   position(ci, x, y, z)           cube ci's position; false if it is no cube of the source (a dense list's always is)
//   locate(x, y, z, home)           where the cube's cells are; false if the source cannot read around it (bricks: its brick is not
//                                   listed).  Two steps, two early returns: one test of both measured an occupancy step lost in
//                                   the soup emit over bricks (profiles/mesh_shared/codegen.txt)
//   corners(home, x, y, z, v, flag) the 8 corner values and their corner_case
//   attributes(home, pos, n, grey)  normal and grey of the vertex at pos
//   slots(tri_offset, t, n_active, ntri, first, planned)   the triangle slots list position t may write: `planned` from `first` on,
//                                   of which a cube with ntri triangles uses min(ntri, planned); false if it has none.  Dense: ntri.
//   VERIFIES_LIST                   whether k_mesh_own looks a cube's neighbours up only once it has found the cube active: the brick
//                                   lists are the caller's device memory; a dense list is the plan's own, and the test costs there
//   owner(cube_index, n_active, t, ci, x, y, z, home, e, oe)   the list position of the cube that owns the lattice edge under edge e
//                                   of the cube at position t, and in oe the edge's number there.  Each source's own rule: the first
//                                   cube around the edge in ITS emission order.

// A listed cube as its thread sees it: position, case, triangle count, the mask of its edges with a vertex, corner values
struct ActiveCube {
    int x, y, z, flag, ntri;
    unsigned mask;
    float v[8];
};

// cube ci; false if the source cannot place or locate it, it has no triangles or a corner that is not finite (a cube of a plan's list over a
// valid source is none of these).  For k_mc_emit_indexed and k_mesh_own; k_mc_emit keeps the same steps in locals.
template <typename SRC>
__device__ __forceinline__ bool active_cube(const SRC& s, long long ci, ActiveCube& c, typename SRC::Home& home)
{
    if (!s.position(ci, c.x, c.y, c.z) || !s.locate(c.x, c.y, c.z, home)) return false;
    const bool finite = s.corners(home, c.x, c.y, c.z, c.v, c.flag);
    c.ntri = c_num_tris[c.flag];
    c.mask = c_edge_mask[c.flag];
    return finite && c.ntri != 0;
}

// The soup: three fresh vertices per triangle of every listed cube.
template <typename SRC>
static __global__ __launch_bounds__(128) void k_mc_emit(const SRC s, const long long* __restrict__ cube_index, const unsigned* __restrict__ tri_offset,
                                                        const long long n_active, float* __restrict__ verts, float* __restrict__ norms,
                                                        float* __restrict__ colors)
{
    const long long t_id = (long long)blockIdx.x * 128 + threadIdx.x;
    if (t_id >= n_active) return;
    // active_cube's steps in locals: through the struct this kernel -- 36 per-edge values live -- compiles to other code, which
    // measured 1 % slower at 1024^3 over a dense volume (profiles/mesh_refactor/ab_timing.txt)
    int x, y, z, flag;
    if (!s.position(cube_index[t_id], x, y, z)) return;
    typename SRC::Home home;
    if (!s.locate(x, y, z, home)) return;
    float v[8];
    if (!s.corners(home, x, y, z, v, flag)) return;
    const int ntri = c_num_tris[flag];
    if (ntri == 0) return;
    const unsigned mask = c_edge_mask[flag];
    const V3 p0 = cube_origin(s.p, x, y, z);
    V3 ev[12], en[12];
    float ec[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        if (!(mask & (1u << e))) continue;
        ev[e] = edge_position(s.p, p0, v, e);
        s.attributes(home, ev[e], en[e], ec[e]);
    }
    unsigned long long first;
    int planned;
    if (!s.slots(tri_offset, t_id, n_active, ntri, first, planned)) return;
    size_t o = (size_t)first * 3; // first output vertex of this cube
    for (int t = 0; t < min(ntri, planned) * 3; ++t, ++o) {
        const int e = c_tris[flag][t];
        V3 P = v3(0.f, 0.f, 0.f), N = P;
        float C = 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k)   // select without dynamic register indexing (one loop for the three arrays: a shared
            if (k == e) { P = ev[k]; N = en[k]; C = ec[k]; }   // per-array select measured slower here, same file)
        store_vertex(verts, norms, colors, o, P, N, C, s.has_color);
    }
}

// info[t] = flag | owned edges << 8; part[2 b] = vertices, part[2 b + 1] = triangles (the slots planned) of block b's cubes.
// hdr[2], hdr[3]: the totals this index was planned for (hdr[0], hdr[1] are the scan's: vertices, triangles).
template <typename SRC>
static __global__ __launch_bounds__(MESH_IDX_BLOCK) void k_mesh_own(const SRC s, const long long* __restrict__ cube_index,
                                                                    const unsigned* __restrict__ tri_offset, const long long n_active,
                                                                    const unsigned long long n_tris, unsigned* __restrict__ info,
                                                                    unsigned* __restrict__ part, unsigned long long* __restrict__ hdr)
{
    static_assert(MESH_IDX_BLOCK == 256, "store_block_sums");
    const long long t = (long long)blockIdx.x * MESH_IDX_BLOCK + threadIdx.x;
    unsigned nv = 0, nt = 0;
    if (t < n_active) {
        const long long ci = cube_index[t];
        ActiveCube c;
        typename SRC::Home home;
        c.flag = c.ntri = 0;   // (of a cube the source cannot locate)
        unsigned own = 0;
        if (active_cube(s, ci, c, home) || !SRC::VERIFIES_LIST) {
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                if (!(c.mask & (1u << e))) continue;
                int oe;
                if (s.owner(cube_index, n_active, t, ci, c.x, c.y, c.z, home, e, oe) == t) own |= 1u << e;
            }
        }
        info[t] = (unsigned)c.flag | (own << 8);
        nv = __popc(own);
        unsigned long long first;
        int planned;
        if (s.slots(tri_offset, t, n_active, c.ntri, first, planned)) nt = (unsigned)planned;
    }
    store_block_sums(nv, nt, part);
    if (threadIdx.x == 0 && blockIdx.x == 0) { hdr[2] = (unsigned long long)n_active; hdr[3] = n_tris; }
}

// k_mc_emit with shared vertices: positions, normals and colours by k_mc_emit's calls, made by the owner only; every triangle
// corner writes base(owner) + rank(edge in owner).  Every vertex id is compared with n_verts before its store.
template <typename SRC>
static __global__ __launch_bounds__(128) void k_mc_emit_indexed(const SRC s, const long long* __restrict__ cube_index,
                                                                const unsigned* __restrict__ tri_offset, const unsigned* __restrict__ info,
                                                                const unsigned* __restrict__ vbase, const long long n_active,
                                                                const unsigned long long n_verts, float* __restrict__ verts,
                                                                float* __restrict__ norms, float* __restrict__ colors, unsigned* __restrict__ faces)
{
    const long long t_id = (long long)blockIdx.x * 128 + threadIdx.x;
    if (t_id >= n_active) return;
    const long long ci = cube_index[t_id];
    ActiveCube c;
    typename SRC::Home home;
    if (!active_cube(s, ci, c, home)) return;
    const unsigned own = info[t_id] >> 8, first_id = vbase[t_id];
    const unsigned long long ranks = edge_ranks(c_tris[c.flag], c.ntri, own);
    const V3 p0 = cube_origin(s.p, c.x, c.y, c.z);
    unsigned id[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        id[e] = 0;
        if (!(c.mask & (1u << e))) continue;
        if (own & (1u << e)) {
            const size_t i = first_id + rank_of(ranks, e);   // (a 32-bit sum: whatever a scratch holds, i is checked next)
            id[e] = (unsigned)i;
            if (i >= n_verts) continue;
            const V3 pos = edge_position(s.p, p0, c.v, e);
            V3 n;
            float grey;
            s.attributes(home, pos, n, grey);
            store_vertex(verts, norms, colors, i, pos, n, grey, s.has_color);
        } else {
            int oe;
            const long long j = s.owner(cube_index, n_active, t_id, ci, c.x, c.y, c.z, home, e, oe);   // (in [0, n_active))
            const unsigned oi = info[j];
            id[e] = vbase[j] + rank_of(edge_ranks(c_tris[oi & 255u], c_num_tris[oi & 255u], oi >> 8), oe);
        }
    }
    unsigned long long first;
    int planned;
    if (!s.slots(tri_offset, t_id, n_active, c.ntri, first, planned)) return;
    size_t o = (size_t)first * 3;   // first face corner of this cube
    for (int t = 0; t < min(c.ntri, planned) * 3; ++t, ++o) {
        const int e = c_tris[c.flag][t];
        unsigned I = 0;
#pragma unroll
        for (int k = 0; k < 12; ++k)   // select without dynamic register indexing
            if (k == e) I = id[k];
        faces[o] = I;
    }
}

// A caller's scratch handed out front to back, every sub-buffer on a 256-byte boundary of it; `bytes` is what has been taken.
// (An integer address: a layout is also carved from a null scratch, for its size alone.)
struct Carver {
    uintptr_t scratch;
    size_t bytes = 0;
    template <typename T> T* take(size_t count)
    {
        T* const at = (T*)(scratch + bytes);
        bytes += (count * sizeof(T) + 255) & ~(size_t)255;
        return at;
    }
};

static bool totals_in_range(const unsigned long long totals[2]) { return totals[1] < MESH_MAX_TRIS && totals[0] <= totals[1]; }

// n 64-bit words of a scratch header, once the stream's earlier work is done
static int read_header(unsigned long long* host, const unsigned long long* dev, int n, hipStream_t st)
{
    hipError_t e = hipMemcpyAsync(host, dev, (size_t)n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : set_error((int)e, hipGetErrorString(e));
}

// "The totals are the plan's": the first n words of a scratch's header are those the caller's totals stand for.  The kernels trust
// the lists planned in that scratch to fit the buffers the caller sized from its totals.
static int check_planned(const unsigned long long* hdr, const unsigned long long* want, int n, const char* what, hipStream_t st)
{
    unsigned long long planned[4];
    if (int e = read_header(planned, hdr, n, st)) return e;
    if (memcmp(planned, want, (size_t)n * 8) != 0) return fail_rule(what, KFX_E_RANGE, "totals are not the plan's");
    return 0;
}

} // namespace kfx
