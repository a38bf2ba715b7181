// mesh.hip -- iso-surface extraction from the TSDF (roo::SaveMesh's marching cubes) for gfx950.
// SURVEY.md 8(f) row f-4.
//
// Reference behaviour: include/kangaroo/MarchingCubes.h:43-143 (vMarchCube: corner values, case index,
// edge vertices by linear interpolation, normals from GetUnitsBackwardDiffDxDyDz, grey colour from the
// colour volume) inside the loop nest of SaveMesh (:226-232: x outer, y, z inner, three fresh vertices per
// triangle).  The reference does this on the host, one cube at a time, after copying the volume back.
//
// Here the volume never leaves HBM.  The cubes are numbered in the REFERENCE's emission order, ci = (x*(h-1) + y)*(d-1) + z, and every
// path ends in one thread per ACTIVE cube (a cube with triangles) whose vertex / normal / colour arithmetic keeps the reference's
// expressions (double division in fGetOffset, multiply-by-reciprocal normalisation): the arrays are bit-identical to the CPU oracle's
// and arrive in the reference's order.  Three paths, each on top of the one before:
//   byte per cube (kfx.h: kfx_mc_count / kfx_mc_emit)   k_mc_count writes every cube's triangle count, the CALLER compacts (prefix sum,
//               non-zero positions) and k_mc_emit writes three vertices per triangle.  fp32, whole volumes; kept as the independent
//               comparator of the tests, and built from nothing the other two share but the corner read and k_mc_emit.
//   soup (kfx_mesh.h: kfx_mesh_plan / kfx_mesh_emit)   what SaveMesh and ExtractMesh call: counts per SEGMENT of a column, scanned and
//               compacted on the device, then k_mc_emit.  fp32 and half cells, whole volumes and Z-slabs.
//   indexed (kfx_mesh_index.h: kfx_mesh_index_plan / kfx_mesh_emit_indexed)   the soup's plan, then its vertices welded by lattice edge:
//               one vertex per edge and a face list, k_mc_emit_indexed.
// k_mc_emit, k_mesh_own, k_mc_emit_indexed, the scan kernel and the case tables are mesh_cube.h's, written over a cube source and
// shared with the extractor of packed bricks (mesh_bricks.hip).  This file has the dense source, DenseCubes -- the corner read from
// pitched rows, the normal and grey with a slab's stored-plane rule, the dense owner rule --, the plan passes over segments of a
// column, the byte-per-cube count, and the host side of the three ABIs.
// The case tables (mc_tables.inc) are derived by scripts/gen_mc_tables.py from the cube's topology; their boundary
// loops and winding equal the classic tables' in all 256 cases (tests/test_mesh_cpu.py).
#define KFX_MESH_UNIT dense_mesh
#include "mesh_cube.h"
#include "../../include/kfx_mesh.h"
#include "../../include/kfx_mesh_index.h"

namespace kfx {

// values at the 8 corners and their corner_case.  Half cells are widened
// exactly (SDF_h's operator float), so a half volume's cubes are those of the widened fp32 volume.
template <typename CELL>
__device__ __forceinline__ bool cube_case(const MeshParams& p, int x, int y, int z, float v[8], int& flag)
{
    const unsigned char* r00 = rowp(p.vol, y, z);
    const unsigned char* r10 = rowp(p.vol, y + 1, z);
    const unsigned char* r01 = rowp(p.vol, y, z + 1);
    const unsigned char* r11 = rowp(p.vol, y + 1, z + 1);
    const float2 a = CELL::pair(r00, x), b = CELL::pair(r10, x), c = CELL::pair(r01, x), d = CELL::pair(r11, x);
    v[0] = a.x; v[1] = a.y; v[2] = b.y; v[3] = b.x;
    v[4] = c.x; v[5] = c.y; v[6] = d.y; v[7] = d.x;
    return corner_case(v, flag);
}

// Workgroup = 64 cubes along x, 16 along z, one y.  Corner rows are read x-fastest (coalesced); the counts go
// through an LDS tile so that each x-row's 16 z-consecutive bytes leave as one segment (the output order is z-fastest).
__global__ __launch_bounds__(256) void k_mc_count(const MeshParams p, unsigned char* __restrict__ counts)
{
    __shared__ unsigned char tile[64][17];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64, y = blockIdx.y, z0 = blockIdx.z * 16;
    const int x = x0 + lane;
    for (int zz = wv; zz < 16; zz += 4) {
        const int z = z0 + zz;
        unsigned char n = 0;
        if (x < p.cx && z < p.cz) {
            float v[8];
            int flag;
            if (cube_case<RayF32>(p, x, y, z, v, flag)) n = c_num_tris[flag];
        }
        tile[lane][zz] = n;
    }
    __syncthreads();
    const int xr = threadIdx.x >> 2, q = threadIdx.x & 3;
    if (x0 + xr < p.cx) {
        unsigned char* dst = counts + ((size_t)(x0 + xr) * p.cy + y) * p.cz;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int z = z0 + q * 4 + b;
            if (z < p.cz) dst[z] = tile[xr][q * 4 + b];
        }
    }
}

// normal and grey colour of the vertex at pos.  SLAB: zero where the planes they read are not stored here
template <typename CELL, bool SLAB>
__device__ __forceinline__ void edge_attributes(const MeshParams& p, const ColorGeom& cv, int has_color, const V3& pos, V3& normal, float& grey)
{
    bool stored = true;   // SLAB: the planes this vertex's normal and colour read are stored here
    V3 n;
    if constexpr (SLAB) {
        // the stencil's planes (gradient<>: base plane clamped to [1, d - 2], one plane either side) must be stored; they are
        // for any vertex within a voxel of its cube, which float positions are unless the box lies ~2^20 voxels from the origin
        const float pfz = (pos.z - p.vol.bmin.z) / p.size.z * p.dims1.z;
        const int iz = (int)fmaxf(fminf(p.hi2.z, floorf(pfz)), 1.f);
        stored = iz - 1 >= p.avail_lo && iz + 1 < p.avail_hi;
        if (stored) {
            const V3 deriv = gradient<CELL>(p, pos);
            n = div_s(deriv, length(deriv));
        } else {
            n = v3(0.f, 0.f, 0.f);
        }
    } else {
        const V3 deriv = gradient<CELL>(p, pos);
        n = div_s(deriv, length(deriv));
    }
    if (!isfinite(n.x) || !isfinite(n.y) || !isfinite(n.z)) n = v3(0.f, 0.f, 0.f);
    normal = n;
    // (SLAB: the colour sample's planes, base clamp(floor(pfz), 0, d - 2) and the next, lie inside the stencil's three: equal geometry)
    grey = (has_color && stored) ? trilinear<RayC32>(cv, pos) : 0.f;
}

// the colour volume of an emit: sampled only when it IsValid(), every dimension >= 8 (BoundedVolume.h:84-87)
static int color_params(ColorGeom& cv, int& has_color, const kfx_volume* colorvol, const float* colors)
{
    cv = ColorGeom{};
    has_color = colorvol && colorvol->ptr && colors && colorvol->w >= 8 && colorvol->h >= 8 && colorvol->d >= 8;
    if (has_color) {
        if (int e = check_volume(colorvol, 4, 8, VOLUME_ANY_DIM, "SaveMesh(colour)")) return e;
        set_geometry(cv, colorvol);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The soup (include/kfx_mesh.h): no array per cube and no compaction by the caller, but four passes over SEGMENTS -- runs of up
// to MESH_SEG consecutive cubes along z in one (x, y) column, numbered in emission order
// s = (x*cy + y)*nsz + k (x outer, z inner: a segment's cubes are consecutive in the reference's order):
//   k_mesh_count     one lane per segment, lanes of a wave on x-adjacent columns (coalesced corner rows); the lane walks z and
//                    keeps plane z+1's corner pairs as the next cube's plane z.  Writes seg_pack(active cubes, triangles), 16 bits.
//   k_mesh_reduce    sums of MESH_BLOCK consecutive segments (the scan's upsweep)
//   k_mesh_scan_partials  mesh_cube.h's: exclusive 64-bit scan of the block sums, and the totals
//   k_mesh_compact   the downsweep inside each block (LDS), then one lane per ACTIVE segment re-walks its cubes and writes the
//                    active cubes' global indices (int64) and first triangles (uint32) at the scanned offsets
//   k_mc_emit        mesh_cube.h's, as kfx_mc_emit
// Kernel boundaries order the passes: no in-launch hand-off between workgroups.
constexpr int MESH_SEG = 64;         // cubes per segment: 8 segments per column at 512^3, 32 at 2048^3
constexpr int MESH_SEG_TILE = 32;    // segments per column and count workgroup (grid z covers the rest)
constexpr int MESH_PER_THREAD = 2;   // segments per thread of the reduce / compact workgroups (small blocks: enough compact waves)
constexpr int MESH_BLOCK = 256 * MESH_PER_THREAD;

struct MeshRange {
    int zlo, zhi;      // cube planes meshed: [zlo, zhi)
    int nsz;           // segments per column
    long long nseg;    // cx * cy * nsz
    long long nblk;    // ceil(nseg / MESH_BLOCK)
};

// a segment's count, 16 bits: active cubes (<= MESH_SEG) above 9 bits of triangles (<= 5 MESH_SEG)
__device__ __forceinline__ unsigned seg_pack(unsigned active, unsigned tris) { return (active << 9) | tris; }
__device__ __forceinline__ unsigned seg_active(unsigned n) { return n >> 9; }
__device__ __forceinline__ unsigned seg_tris(unsigned n) { return n & 511u; }

// The cubes [za, zb) of column (x, y) from the bottom up, plane z + 1's corner pairs kept as the next cube's plane z: each(z, n)
// gets every cube's plane and triangle count.  Plan and emit both walk with this, so they agree on which cubes are active.
template <typename CELL, typename F>
__device__ __forceinline__ void walk_segment(const MeshParams& p, int x, int y, int za, int zb, F each)
{
    float2 a = CELL::pair(rowp(p.vol, y, za), x), b = CELL::pair(rowp(p.vol, y + 1, za), x);
    for (int z = za; z < zb; ++z) {
        const float2 c = CELL::pair(rowp(p.vol, y, z + 1), x), d = CELL::pair(rowp(p.vol, y + 1, z + 1), x);
        const float v[8] = {a.x, a.y, b.y, b.x, c.x, c.y, d.y, d.x};   // cube_case's corner order
        int flag;
        each(z, corner_case(v, flag) ? c_num_tris[flag] : 0u);
        a = c;
        b = d;
    }
}

// active cubes and triangles of the cubes [za, zb) of column (x, y)
template <typename CELL>
__device__ __forceinline__ unsigned segment_count(const MeshParams& p, int x, int y, int za, int zb)
{
    unsigned active = 0, tris = 0;
    walk_segment<CELL>(p, x, y, za, zb, [&](int, unsigned n) {
        active += n != 0;
        tris += n;
    });
    return seg_pack(active, tris);
}

// Workgroup = 64 columns along x (one per lane) x MESH_SEG_TILE segments of one y; wave w takes segments w, w + 4, ...  The
// counts leave through an LDS tile so that each column's segments (consecutive in emission order) are stored together.
template <typename CELL>
__global__ __launch_bounds__(256) void k_mesh_count(const MeshParams p, const MeshRange r, unsigned short* __restrict__ seg)
{
    __shared__ unsigned short tile[64][MESH_SEG_TILE + 2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = blockIdx.x * 64, y = blockIdx.y, k0 = blockIdx.z * MESH_SEG_TILE;
    const int x = x0 + lane;
    for (int kk = wv; kk < MESH_SEG_TILE; kk += 4) {
        const int k = k0 + kk;
        unsigned n = 0;
        if (x < p.cx && k < r.nsz) {
            const int za = r.zlo + k * MESH_SEG;
            n = segment_count<CELL>(p, x, y, za, min(za + MESH_SEG, r.zhi));
        }
        tile[lane][kk] = (unsigned short)n;
    }
    __syncthreads();
    // 4 threads per column, each MESH_SEG_TILE / 4 consecutive segments
    const int xr = threadIdx.x >> 2, q = threadIdx.x & 3;
    if (x0 + xr < p.cx) {
        unsigned short* dst = seg + ((long long)(x0 + xr) * p.cy + y) * r.nsz;
#pragma unroll
        for (int b = 0; b < MESH_SEG_TILE / 4; ++b) {
            const int kk = q * (MESH_SEG_TILE / 4) + b, k = k0 + kk;
            if (k < r.nsz) dst[k] = tile[xr][kk];
        }
    }
}

// sums of MESH_BLOCK consecutive segments: part[2 b] = active cubes, part[2 b + 1] = triangles
__global__ __launch_bounds__(256) void k_mesh_reduce(const unsigned short* __restrict__ seg, const MeshRange r, unsigned* __restrict__ part)
{
    const long long s0 = (long long)blockIdx.x * MESH_BLOCK + (long long)threadIdx.x * MESH_PER_THREAD;
    unsigned a = 0, t = 0;
    for (int j = 0; j < MESH_PER_THREAD; ++j) {
        const unsigned n = s0 + j < r.nseg ? seg[s0 + j] : 0u;
        a += seg_active(n);
        t += seg_tris(n);
    }
    store_block_sums(a, t, part);
}

// One workgroup per block of MESH_BLOCK segments: the block's exclusive offsets in LDS (thread t scans its MESH_PER_THREAD
// consecutive segments, the workgroup scans the threads' sums), then lane t walks segments t, t + 256, ... that have active
// cubes and writes each active cube's global index and first triangle.  Writes stop at the caller's capacities.
template <typename CELL>
__global__ __launch_bounds__(256) void k_mesh_compact(const MeshParams p, const MeshRange r, const unsigned short* __restrict__ seg,
                                                      const unsigned long long* __restrict__ base, long long* __restrict__ cube_index,
                                                      unsigned* __restrict__ tri_offset, const unsigned long long cap_active,
                                                      const unsigned long long cap_tris)
{
    __shared__ unsigned off_a[MESH_BLOCK], off_t[MESH_BLOCK];
    __shared__ unsigned short cnt[MESH_BLOCK];
    __shared__ unsigned lds[2][4];
    const long long blk0 = (long long)blockIdx.x * MESH_BLOCK;
    const int j0 = threadIdx.x * MESH_PER_THREAD;
    unsigned sa = 0, st = 0;
    for (int j = 0; j < MESH_PER_THREAD; ++j) {
        const unsigned short n = blk0 + j0 + j < r.nseg ? seg[blk0 + j0 + j] : (unsigned short)0;
        cnt[j0 + j] = n;
        sa += seg_active(n);
        st += seg_tris(n);
    }
    unsigned ta, tt;
    unsigned ea = block_exclusive_scan<unsigned, 4>(sa, lds[0], &ta);
    unsigned et = block_exclusive_scan<unsigned, 4>(st, lds[1], &tt);
    for (int j = 0; j < MESH_PER_THREAD; ++j) {
        off_a[j0 + j] = ea;
        off_t[j0 + j] = et;
        ea += seg_active(cnt[j0 + j]);
        et += seg_tris(cnt[j0 + j]);
    }
    __syncthreads();
    const unsigned long long ba = base[2 * (size_t)blockIdx.x], bt = base[2 * (size_t)blockIdx.x + 1];
    for (int j = threadIdx.x; j < MESH_BLOCK; j += 256) {
        if (cnt[j] == 0) continue;
        const long long s = blk0 + j;
        const long long col = s / r.nsz;
        const int k = (int)(s - col * r.nsz);
        const int x = (int)(col / p.cy), y = (int)(col - (long long)x * p.cy);
        const int za = r.zlo + k * MESH_SEG, zb = min(za + MESH_SEG, r.zhi);
        unsigned long long ia = ba + off_a[j], it = bt + off_t[j];
        const long long ci0 = col * p.cz;
        walk_segment<CELL>(p, x, y, za, zb, [&](int z, unsigned n) {
            if (!n) return;
            if (ia < cap_active && it + n <= cap_tris) {
                cube_index[ia] = ci0 + z;
                tri_offset[ia] = (unsigned)it;
            }
            ++ia;
            it += n;
        });
    }
}

// The meshed cube planes and the geometry: the whole volume, or a slab view through the full volume's geometry
// (slab_full_volume: the virtual base pointer is dereferenced only inside the stored planes).
static int mesh_setup(MeshParams& p, MeshRange& r, const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi)
{
    if (!vol || !vol->ptr) return set_error(KFX_E_NULL, "kfx_mesh: null volume");
    if (cell != KFX_CELL_F32 && cell != KFX_CELL_F16) return set_error(KFX_E_RANGE, "kfx_mesh: unknown cell kind");
    const size_t cb = cell == KFX_CELL_F32 ? 8 : 4;
    kfx_volume full = *vol;   // the volume the cubes are numbered in
    if (!slab) {
        if (int e = check_volume(vol, cb, 3, VOLUME_MAX_DIM, "SaveMesh")) return e;
        r.zlo = 0;
        r.zhi = (int)vol->d - 1;
    } else {
        // (a slab may store a single plane; w and h as for a whole volume)
        if (vol->w < 3 || vol->h < 3 || slab->full_d < 3 || slab->full_d > 65535 || slab->z_offset + vol->d > slab->full_d)
            return set_error(KFX_E_SHAPE, "kfx_mesh: slab outside the full volume");
        if (int e = check_volume(vol, cb, 1, VOLUME_MAX_DIM, "kfx_mesh(slab)")) return e;
        const int full_d = (int)slab->full_d;
        const int zlo = own_lo < 0 ? 0 : own_lo, zhi = own_hi < full_d - 1 ? own_hi : full_d - 1;
        r.zlo = zlo;
        r.zhi = zhi > zlo ? zhi : zlo;
        if (r.zhi > r.zlo) {
            // corners: planes z, z + 1; normals: gradient<>'s base plane clamp(floor(vertex z), 1, d - 2), with the vertex in
            // [z, z + 1], and its planes either side -> [zlo - 2, zhi + 2) within the volume
            const long long need_lo = r.zlo - 2 > 0 ? r.zlo - 2 : 0, need_hi = r.zhi + 2 < full_d ? r.zhi + 2 : full_d;
            if (need_lo < (long long)slab->z_offset || need_hi > (long long)(slab->z_offset + vol->d))
                return set_error(KFX_E_RANGE, "kfx_mesh: the stored planes do not cover the slab's cubes and their normals' stencil");
        }
        full = slab_full_volume(vol, slab);
    }
    set_geometry(p, &full);
    set_voxel_size(p, &full);
    p.cx = (int)full.w - 1; p.cy = (int)full.h - 1; p.cz = (int)full.d - 1;
    p.avail_lo = slab ? (int)slab->z_offset : 0;
    p.avail_hi = p.avail_lo + (int)vol->d;
    r.nsz = (r.zhi - r.zlo + MESH_SEG - 1) / MESH_SEG;
    r.nseg = (long long)p.cx * p.cy * r.nsz;
    r.nblk = (r.nseg + MESH_BLOCK - 1) / MESH_BLOCK;
    return 0;
}

// scratch: [header: totals][segment counts, 2 B, nblk * MESH_BLOCK][block sums, 8 B per block][block offsets, 16 B per block]
struct MeshScratch {
    unsigned long long* totals;
    unsigned short* seg;
    unsigned* part;
    unsigned long long* base;
    size_t bytes;
};
static MeshScratch mesh_scratch(const MeshRange& r, const void* scratch)
{
    Carver c{(uintptr_t)scratch};
    MeshScratch s;
    s.totals = c.take<unsigned long long>(MESH_HEADER / 8);
    s.seg = c.take<unsigned short>((size_t)r.nblk * MESH_BLOCK);
    s.part = c.take<unsigned>((size_t)r.nblk * 2);
    s.base = c.take<unsigned long long>((size_t)r.nblk * 2);
    s.bytes = c.bytes;
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Indexed extraction (include/kfx_mesh_index.h): the soup welded by LATTICE EDGE -- (minimum corner, axis) of the cube edge a
// vertex lies on -- into the sequential first-occurrence mesh.  A lattice edge belongs to up to four cubes; its OWNER is the first
// of them in emission order that is meshed.  A cube with a sign change on an edge and eight finite corners has triangles, so
// "meshed" is "listed in cube_index", answered by a binary search in the compacted, ascending list: no table per voxel or edge.
//   k_mesh_compact      as above, into the index scratch
//   k_mesh_own          one lane per active cube: case flag and the 12-bit mask of the edges it owns (4 bytes), block sums
//   k_mesh_scan_partials   as above: the blocks' first vertex ids, the vertex total
//   k_mesh_vertex_base  every active cube's first vertex id (4 bytes)
//   k_mc_emit_indexed   one lane per active cube: owned edges write their vertex at base + rank, rank = first use among the owned
//                       edges in c_tris[flag]; every triangle corner writes base(owner) + rank(edge in owner)
// All but k_mesh_compact are mesh_cube.h's, as is how an edge is named in its owner and ranked among the owner's edges: the index of
// packed bricks (mesh_bricks.hip) differs in the owner rule alone.  The dense rule is edge_owner, below.

// position of cube c in the ascending cube_index[0, n), -1 if it is not listed
__device__ __forceinline__ long long find_cube(const long long* __restrict__ cube_index, long long n, long long c)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (cube_index[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && cube_index[lo] == c ? lo : -1;
}

// The owner of the lattice edge under edge e of active cube t = (x, y, z), index ci: its position in cube_index, and in oe the
// edge's number there.  The edge's axis is a; along the other two axes u < w (x before y before z: the emission order's
// significance) the four cubes around it sit at the edge's minimum corner minus (su, sw) in {0, 1}^2, this cube at its own
// minimum-corner offsets (mesh_cube.h: lattice_edge).  The candidates before this cube are looked up in ascending order; without one the cube owns the edge.
__device__ __forceinline__ long long edge_owner(const MeshParams& p, const long long* __restrict__ cube_index, long long t, long long ci,
                                                int x, int y, int z, int e, int& oe)
{
    const LatticeEdge l = lattice_edge(e);
    const int a = l.a, u = l.u, w = l.w;
    const int* const m = l.m;
    const int at[3] = {x, y, z}, cubes[3] = {p.cx, p.cy, p.cz};
    const long long stride[3] = {(long long)p.cy * p.cz, (long long)p.cz, 1};
#pragma unroll
    for (int su = 1; su >= 0; --su) {
#pragma unroll
        for (int sw = 1; sw >= 0; --sw) {
            const int du = m[u] - su, dw = m[w] - sw;
            if (!(du < 0 || (du == 0 && dw < 0))) continue;   // this cube or a later one
            const int nu = at[u] + du, nw = at[w] + dw;
            if (nu < 0 || nu >= cubes[u] || nw < 0 || nw >= cubes[w]) continue;
            const long long j = find_cube(cube_index, t, ci + du * stride[u] + dw * stride[w]);
            if (j >= 0) {
                // the edge of axis a with minimum corner (su, sw) in the owner
                oe = owner_e(a, su, sw);
                return j;
            }
        }
    }
    oe = e;
    return t;
}

// The dense volume as mesh_cube.h's cube source: every listed cube can be read.  CELL: fp32 or half cells; SLAB: p holds the full
// volume's geometry over a slab's planes [avail_lo, avail_hi) (virtual base pointer, slab_full_volume), and so does cv for the rank's
// colour slab, which has the SDF slab's geometry.
template <typename CELL, bool SLAB>
struct DenseCubes {
    MeshParams p;
    ColorGeom cv;
    int has_color;
    struct Home {};
    static constexpr bool VERIFIES_LIST = false;
    __device__ __forceinline__ bool position(long long ci, int& x, int& y, int& z) const
    {
        cube_xyz(p, ci, x, y, z);
        return true;
    }
    __device__ __forceinline__ bool locate(int, int, int, Home&) const { return true; }
    __device__ __forceinline__ bool corners(const Home&, int x, int y, int z, float v[8], int& flag) const { return cube_case<CELL>(p, x, y, z, v, flag); }
    __device__ __forceinline__ void attributes(const Home&, const V3& pos, V3& normal, float& grey) const
    {
        edge_attributes<CELL, SLAB>(p, cv, has_color, pos, normal, grey);
    }
    // (the plan counted this cube from these cells: its slots are its triangles)
    __device__ __forceinline__ bool slots(const unsigned* tri_offset, long long t, long long, int ntri, unsigned long long& first, int& planned) const
    {
        first = tri_offset[t];
        planned = ntri;
        return true;
    }
    __device__ __forceinline__ long long owner(const long long* cube_index, long long, long long t, long long ci, int x, int y, int z, const Home&,
                                               int e, int& oe) const
    {
        return edge_owner(p, cube_index, t, ci, x, y, z, e, oe);
    }
};

// index scratch: [header: vertices, triangles, planned cubes, planned triangles][cube_index, 8 B][tri_offset, 4 B][info, 4 B]
// [vbase, 4 B] per active cube, [block sums, 8 B][block offsets, 16 B] per MESH_IDX_BLOCK active cubes
struct MeshIndexScratch {
    unsigned long long* hdr;
    long long* cube_index;
    unsigned *tri_offset, *info, *vbase, *part;
    unsigned long long* base;
    long long nblk;
    size_t bytes;
};
static MeshIndexScratch mesh_index_scratch(unsigned long long n_active, const void* scratch)
{
    Carver c{(uintptr_t)scratch};
    MeshIndexScratch s;
    s.nblk = (long long)((n_active + MESH_IDX_BLOCK - 1) / MESH_IDX_BLOCK);
    s.hdr = c.take<unsigned long long>(MESH_HEADER / 8);
    s.cube_index = c.take<long long>((size_t)n_active);
    s.tri_offset = c.take<unsigned>((size_t)n_active);
    s.info = c.take<unsigned>((size_t)n_active);
    s.vbase = c.take<unsigned>((size_t)n_active);
    s.part = c.take<unsigned>((size_t)s.nblk * 2);
    s.base = c.take<unsigned long long>((size_t)s.nblk * 2);
    s.bytes = c.bytes;
    return s;
}

// the colour volume of a soup or indexed emit (kfx_mesh.h: colorvol)
static int mesh_color_params(ColorGeom& cv, int& has_color, const kfx_volume* vol, int cell, const kfx_slab* slab, const kfx_volume* colorvol,
                             const float* colors)
{
    has_color = 0;
    if (!slab) {
        if (int e = color_params(cv, has_color, colorvol, colors)) return e;
    } else if (colorvol && colorvol->ptr && colors) {
        // the rank's colour slab: the planes of `vol` of a colour volume with the SDF volume's geometry, seen through the full volume
        if (cell != KFX_CELL_F32) return set_error(KFX_E_RANGE, "kfx_mesh_emit: colour on slabs needs fp32 SDF cells");
        if (int e = check_volume(colorvol, 4, 1, VOLUME_ANY_DIM, "SaveMesh(colour, slab)")) return e;
        if (int e = check_color_slab(vol, colorvol, "SaveMesh(colour, slab)")) return e;
        const kfx_volume cfull = slab_full_volume(colorvol, slab);
        if (int e = color_params(cv, has_color, &cfull, colors)) return e;   // (IsValid() of the FULL colour volume)
    }
    if (!has_color) cv = ColorGeom{};
    return 0;
}

// How the entry points of kfx_mesh.h and kfx_mesh_index.h open: the geometry, the meshed range and the carved scratches of a call
// that `takes` a plan's scratch, an index scratch (sizing: null, SIZE_MAX bytes), totals of the caller's.  The checks come in one
// order, which the code of a refusal depends on: the volume and the slab (mesh_setup); the entry point's pointers (`any_null`); with
// an index scratch, whose layout they decide, the totals' range (and n_verts <= 3 triangles); the scratches' alignment; their sizes;
// without an index scratch, the totals' range.
enum { MESH_PLAN_SCRATCH = 1, MESH_INDEX_SCRATCH = 2, MESH_TOTALS = 4 };
struct MeshCall {
    MeshParams p;
    MeshRange r;
    MeshScratch s;        // with MESH_PLAN_SCRATCH
    MeshIndexScratch x;   // with MESH_INDEX_SCRATCH
};
static int mesh_call(MeshCall& c, const char* what, int takes, const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi,
                     bool any_null, const void* scratch, size_t scratch_bytes, const void* index_scratch, size_t index_scratch_bytes,
                     const unsigned long long* totals, unsigned long long n_verts = 0)
{
    if (int e = mesh_setup(c.p, c.r, vol, cell, slab, own_lo, own_hi)) return e;
    if (any_null) return fail_rule(what, KFX_E_NULL, "null scratch, totals or count");
    const bool plan = takes & MESH_PLAN_SCRATCH, index = takes & MESH_INDEX_SCRATCH;
    if (index && (!totals_in_range(totals) || n_verts > 3 * totals[1])) return fail_rule(what, KFX_E_RANGE, "totals out of range");
    if (((plan ? (uintptr_t)scratch : 0) | (index ? (uintptr_t)index_scratch : 0)) & 255)
        return fail_rule(what, KFX_E_ALIGN, "scratch not 256-byte aligned");
    if (plan) c.s = mesh_scratch(c.r, scratch);
    if (index) c.x = mesh_index_scratch(totals[0], index_scratch);
    if (plan && scratch_bytes < c.s.bytes) return fail_rule(what, KFX_E_SHAPE, "scratch smaller than kfx_mesh_scratch_bytes");
    if (index && index_scratch_bytes < c.x.bytes) return fail_rule(what, KFX_E_SHAPE, "index scratch smaller than kfx_mesh_index_scratch_bytes");
    if (!index && (takes & MESH_TOTALS) && !totals_in_range(totals)) return fail_rule(what, KFX_E_RANGE, "totals out of range");
    return 0;
}

// One call of f with the tag of a (cell, slab) pair: the template arguments of the kernels
template <typename CELL_, bool SLAB> struct MeshKind { using CELL = CELL_; using Cubes = DenseCubes<CELL_, SLAB>; };
template <typename F>
static void for_mesh_kind(int cell, bool slab, F f)
{
    if (cell == KFX_CELL_F32 && slab) f(MeshKind<RayF32, true>{});
    else if (cell == KFX_CELL_F32) f(MeshKind<RayF32, false>{});
    else if (slab) f(MeshKind<RayF16, true>{});
    else f(MeshKind<RayF16, false>{});
}

} // namespace kfx

using namespace kfx;

extern "C" int kfx_mc_count(const kfx_volume* vol, unsigned char* counts, kfx_stream stream)
{
    MeshParams p;
    MeshRange r;
    if (int e = mesh_setup(p, r, vol, KFX_CELL_F32, nullptr, 0, 0)) return e;
    if (!counts) return set_error(KFX_E_NULL, "SaveMesh: null counts");
    if (int e = load_tables()) return e;
    dim3 grid(ceil_div(p.cx, 64), p.cy, ceil_div(p.cz, 16));
    hipLaunchKernelGGL(k_mc_count, grid, dim3(256), 0, (hipStream_t)stream, p, counts);
    return check_launch("kfx_mc_count");
}

extern "C" int kfx_mc_emit(const kfx_volume* vol, const kfx_volume* colorvol, const long long* cube_index, const unsigned* tri_offset,
                           long long n_active, float* verts, float* norms, float* colors, kfx_stream stream)
{
    MeshParams p;
    MeshRange r;
    if (int e = mesh_setup(p, r, vol, KFX_CELL_F32, nullptr, 0, 0)) return e;
    if (n_active <= 0) return 0;
    if (!cube_index || !tri_offset || !verts || !norms) return set_error(KFX_E_NULL, "SaveMesh: null output");
    if (int e = load_tables()) return e;
    ColorGeom cv;
    int has_color = 0;
    if (int e = color_params(cv, has_color, colorvol, colors)) return e;
    if (n_active > 0x7fffffffLL * 128) return set_error(KFX_E_RANGE, "SaveMesh: too many active cubes");
    using Cubes = DenseCubes<RayF32, false>;
    hipLaunchKernelGGL(k_mc_emit<Cubes>, dim3((unsigned)((n_active + 127) / 128)), dim3(128), 0, (hipStream_t)stream, (Cubes{p, cv, has_color}),
                       cube_index, tri_offset, n_active, verts, norms, colors);
    return check_launch("kfx_mc_emit");
}

extern "C" size_t kfx_mesh_scratch_bytes(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi)
{
    MeshParams p;
    MeshRange r;
    if (mesh_setup(p, r, vol, cell, slab, own_lo, own_hi)) return 0;
    return mesh_scratch(r, nullptr).bytes;
}

extern "C" int kfx_mesh_plan(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi, void* scratch,
                             size_t scratch_bytes, unsigned long long totals[2], kfx_stream stream)
{
    MeshCall c;
    if (int e = mesh_call(c, "kfx_mesh_plan", MESH_PLAN_SCRATCH, vol, cell, slab, own_lo, own_hi, !scratch || !totals, scratch, scratch_bytes,
                          nullptr, 0, nullptr))
        return e;
    const MeshParams& p = c.p;
    const MeshRange& r = c.r;
    const MeshScratch& s = c.s;
    if (r.nblk > 0x7fffffffLL) return set_error(KFX_E_RANGE, "kfx_mesh_plan: volume too large");
    totals[0] = totals[1] = 0;
    if (r.nseg == 0) return 0;
    if (int e = load_tables()) return e;
    const hipStream_t st = (hipStream_t)stream;
    for_mesh_kind(cell, false, [&](auto kind) {   // (the plan's kernels see a slab through p and r alone)
        using CELL = typename decltype(kind)::CELL;
        dim3 grid(ceil_div(p.cx, 64), p.cy, ceil_div(r.nsz, MESH_SEG_TILE));
        hipLaunchKernelGGL(k_mesh_count<CELL>, grid, dim3(256), 0, st, p, r, s.seg);
        hipLaunchKernelGGL(k_mesh_reduce, dim3((unsigned)r.nblk), dim3(256), 0, st, s.seg, r, s.part);
        hipLaunchKernelGGL(k_mesh_scan_partials, dim3(1), dim3(MESH_SCAN_THREADS), 0, st, s.part, r.nblk, s.base, s.totals);
    });
    if (int e = check_launch("kfx_mesh_plan")) return e;
    unsigned long long host[2];
    if (int e = read_header(host, s.totals, 2, st)) return e;
    totals[0] = host[0];
    totals[1] = host[1];
    if (totals[1] >= MESH_MAX_TRIS) return set_error(KFX_E_RANGE, "kfx_mesh_plan: 2^32/3 triangles or more (32-bit vertex offsets)");
    return 0;
}

extern "C" int kfx_mesh_emit(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi, const kfx_volume* colorvol,
                             const void* scratch, size_t scratch_bytes, const unsigned long long totals[2], long long* cube_index,
                             unsigned* tri_offset, float* verts, float* norms, float* colors, kfx_stream stream)
{
    MeshCall c;
    if (int e = mesh_call(c, "kfx_mesh_emit", MESH_PLAN_SCRATCH | MESH_TOTALS, vol, cell, slab, own_lo, own_hi, !scratch || !totals, scratch,
                          scratch_bytes, nullptr, 0, totals))
        return e;
    if (totals[0] == 0) return 0;
    if (!cube_index || !tri_offset || !verts || !norms) return set_error(KFX_E_NULL, "kfx_mesh_emit: null output");
    if ((((uintptr_t)cube_index) & 7) || (((uintptr_t)tri_offset | (uintptr_t)verts | (uintptr_t)norms | (uintptr_t)colors) & 3))
        return set_error(KFX_E_ALIGN, "kfx_mesh_emit: output alignment");
    ColorGeom cv;
    int has_color = 0;
    if (int e = mesh_color_params(cv, has_color, vol, cell, slab, colorvol, colors)) return e;
    if (int e = load_tables()) return e;
    const hipStream_t st = (hipStream_t)stream;
    if (int e = check_planned(c.s.totals, totals, 2, "kfx_mesh_emit", st)) return e;
    const long long n_active = (long long)totals[0];
    // Every (cell, slab) gets has_color as computed and the colours pointer only with it.  The launches once differed in this arm
    // by arm (a literal 0 for half-cell slabs, `colors` as passed for whole volumes) without a difference in effect:
    // mesh_color_params has refused colour on half-cell slabs, and the kernels write colours only under has_color.
    for_mesh_kind(cell, slab != nullptr, [&](auto kind) {
        using K = decltype(kind);
        hipLaunchKernelGGL(k_mesh_compact<typename K::CELL>, dim3((unsigned)c.r.nblk), dim3(256), 0, st, c.p, c.r, c.s.seg, c.s.base, cube_index,
                           tri_offset, totals[0], totals[1]);
        hipLaunchKernelGGL(k_mc_emit<typename K::Cubes>, dim3((unsigned)((n_active + 127) / 128)), dim3(128), 0, st,
                           (typename K::Cubes{c.p, cv, has_color}), cube_index, tri_offset, n_active, verts, norms, has_color ? colors : nullptr);
    });
    return check_launch("kfx_mesh_emit");
}

// ---- indexed extraction (include/kfx_mesh_index.h) ----

extern "C" size_t kfx_mesh_index_scratch_bytes(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi,
                                               const unsigned long long totals[2])
{
    MeshCall c;
    if (mesh_call(c, "kfx_mesh_index_scratch_bytes", MESH_INDEX_SCRATCH, vol, cell, slab, own_lo, own_hi, !totals, nullptr, 0, nullptr, SIZE_MAX, totals))
        return 0;
    return c.x.bytes;
}

extern "C" int kfx_mesh_index_plan(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi, const void* scratch,
                                   size_t scratch_bytes, const unsigned long long totals[2], void* index_scratch,
                                   size_t index_scratch_bytes, unsigned long long* n_verts, kfx_stream stream)
{
    MeshCall c;
    if (int e = mesh_call(c, "kfx_mesh_index_plan", MESH_PLAN_SCRATCH | MESH_INDEX_SCRATCH, vol, cell, slab, own_lo, own_hi,
                          !scratch || !totals || !index_scratch || !n_verts, scratch, scratch_bytes, index_scratch, index_scratch_bytes, totals))
        return e;
    const MeshIndexScratch& x = c.x;
    *n_verts = 0;
    if (totals[0] == 0) return 0;
    if (int e = load_tables()) return e;
    const hipStream_t st = (hipStream_t)stream;
    if (int e = check_planned(c.s.totals, totals, 2, "kfx_mesh_index_plan", st)) return e;
    const long long n_active = (long long)totals[0];
    for_mesh_kind(cell, false, [&](auto kind) {   // (as the plan's)
        using CELL = typename decltype(kind)::CELL;
        hipLaunchKernelGGL(k_mesh_compact<CELL>, dim3((unsigned)c.r.nblk), dim3(256), 0, st, c.p, c.r, c.s.seg, c.s.base, x.cube_index,
                           x.tri_offset, totals[0], totals[1]);
        using Cubes = DenseCubes<CELL, false>;
        hipLaunchKernelGGL(k_mesh_own<Cubes>, dim3((unsigned)x.nblk), dim3(MESH_IDX_BLOCK), 0, st, (Cubes{c.p, ColorGeom{}, 0}), x.cube_index,
                           x.tri_offset, n_active, totals[1], x.info, x.part, x.hdr);
        hipLaunchKernelGGL(k_mesh_scan_partials, dim3(1), dim3(MESH_SCAN_THREADS), 0, st, x.part, x.nblk, x.base, x.hdr);
        hipLaunchKernelGGL(k_mesh_vertex_base, dim3((unsigned)x.nblk), dim3(MESH_IDX_BLOCK), 0, st, x.info, n_active, x.base, x.vbase);
    });
    if (int e = check_launch("kfx_mesh_index_plan")) return e;
    unsigned long long host[2];
    if (int e = read_header(host, x.hdr, 2, st)) return e;
    *n_verts = host[0];
    return 0;
}

extern "C" int kfx_mesh_emit_indexed(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi, const kfx_volume* colorvol,
                                     const void* index_scratch, size_t index_scratch_bytes, const unsigned long long totals[2],
                                     unsigned long long n_verts, float* verts, float* norms, float* colors, unsigned* faces, kfx_stream stream)
{
    MeshCall c;
    if (int e = mesh_call(c, "kfx_mesh_emit_indexed", MESH_INDEX_SCRATCH, vol, cell, slab, own_lo, own_hi, !index_scratch || !totals, nullptr, 0,
                          index_scratch, index_scratch_bytes, totals, n_verts))
        return e;
    const MeshIndexScratch& x = c.x;
    if (totals[0] == 0) return 0;
    if (!verts || !norms || !faces) return set_error(KFX_E_NULL, "kfx_mesh_emit_indexed: null output");
    if (((uintptr_t)verts | (uintptr_t)norms | (uintptr_t)colors | (uintptr_t)faces) & 3) return set_error(KFX_E_ALIGN, "kfx_mesh_emit_indexed: output alignment");
    ColorGeom cv;
    int has_color = 0;
    if (int e = mesh_color_params(cv, has_color, vol, cell, slab, colorvol, colors)) return e;
    if (int e = load_tables()) return e;
    const hipStream_t st = (hipStream_t)stream;
    // (the index plan's header: vertices, triangles, and the totals it was planned for)
    const unsigned long long planned[4] = {n_verts, totals[1], totals[0], totals[1]};
    if (int e = check_planned(x.hdr, planned, 4, "kfx_mesh_emit_indexed", st)) return e;
    const long long n_active = (long long)totals[0];
    for_mesh_kind(cell, slab != nullptr, [&](auto kind) {   // (colours: as kfx_mesh_emit)
        using K = decltype(kind);
        hipLaunchKernelGGL(k_mc_emit_indexed<typename K::Cubes>, dim3((unsigned)((n_active + 127) / 128)), dim3(128), 0, st,
                           (typename K::Cubes{c.p, cv, has_color}), x.cube_index, x.tri_offset, x.info, x.vbase, n_active, n_verts, verts, norms,
                           has_color ? colors : nullptr, faces);
    });
    return check_launch("kfx_mesh_emit_indexed");
}
