// mesh_cube.h -- what the marching-cubes extractors share: the dense volume's (mesh.hip: kfx_mc_*, kfx_mesh_*, kfx_mesh_index_*) and the
// packed bricks' (mesh_bricks.hip: kfx_mesh_bricks_*).  The case tables, a cube's corners and case, a vertex's position on its edge,
// the normalisation of its normal and its store -- one definition each, so that a brick mesh stays the dense mesh of the volume its
// bricks unpack into, bit for bit -- and the host helpers of the two-step calls: the scratch carver, the scan of the block sums, the
// read-back of a plan's totals; and of the two indexed extractions how a lattice edge is named in its owner, how a cube ranks the edges
// it owns, and the kernel that turns the owned-edge counts into first vertex ids.  How a CELL is read (pitched rows, or bricks through
// a neighbour table) is the including file's.
#pragma once

#include "kfx_device.h"
#include "sampling.h"
#include "host_args.h"
#include "block_scan.h"

namespace kfx {

// (the case tables -- mc_tables.inc in __constant__ memory -- are each translation unit's own: a device symbol belongs to one code object)
#include "mc_tables.inc"

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

// one workgroup of MESH_SCAN_THREADS: exclusive 64-bit offsets of the blocks (base[2 b] cubes, base[2 b + 1] triangles) and the
// totals; the body of each file's scan kernel
__device__ __forceinline__ void scan_block_sums(const unsigned* __restrict__ part, const long long nblk, unsigned long long* __restrict__ base,
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
