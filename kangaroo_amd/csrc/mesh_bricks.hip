// mesh_bricks.hip -- marching cubes straight from packed 8 x 8 x 8 bricks (include/kfx_mesh_bricks.h): the mesh of a FRAME, a virtual
// dense volume of which only the listed bricks exist and every other cell is NaN (colour: 0.5), without that volume.  The result is
// the dense extractor's (mesh.hip) on the volume the bricks would unpack into, bit for bit, because the kernels that make vertices
// and faces are the dense extractor's own: mesh_cube.h's k_mc_emit, k_mesh_own and k_mc_emit_indexed, instantiated here over
// BrickCubes, the cube source that reads a cube's cells through the brick lists.  The frame's geometry is a MeshParams filled by the
// same set_geometry; the gradient stencil and the colour blend are sampling.h's own (gradient_over, trilinear_over: the dense
// samplers' base cell and blend) over BrickCells.  This file has that source -- with the slot clamp and the brick owner rule --, the
// plan passes over bricks, and the host side of the two ABIs.
//
//   k_bm_neighbours   one lane per (listed brick, neighbour): the neighbour's position in the ascending id list by binary search, -1
//                     if absent -- 27 positions per brick, the brick's own among them.  After this a frame cell within 8 cells of a
//                     brick is two dependent loads away.  The same kernel maps the SDF list's neighbours into the colour list.
//   k_bm_count        one workgroup per listed brick: its 9 x 9 x 9 corner values in LDS (2916 bytes) -- its own 8^3 by one 16- / 8-byte
//                     load per lane, the +1 faces, edges and corner from up to seven neighbours -- then two cubes per lane, those
//                     inside the frame's (w - 1, h - 1, d - 1); active cubes and triangles of the brick, 4 bytes.
//   k_bm_reduce, k_mesh_scan_partials   sums of 256 bricks, their exclusive offsets and the totals (mesh_cube.h's scan)
//   k_bm_compact      one workgroup per listed brick with cubes: stages and classifies again, ranks its active cubes in dense order
//                     (lane t holds cubes 2 t, 2 t + 1 of the brick in x-major order = ascending ci) and writes cube_index / tri_offset
//   k_mc_emit         mesh_cube.h's, one lane per ACTIVE cube: the cube's brick by binary search (BrickCubes::locate), corners and
//                     stencils through the neighbour table
//   k_bm_first, k_mesh_own, k_mc_emit_indexed   the indexed output (include/kfx_mesh_bricks_index.h): that soup welded by lattice
//                     edge; described above k_bm_first
// Memory: the lists, about 112 (colour: 220) bytes of scratch per listed brick, the outputs; with the index 20 bytes per active cube
// and 4 per listed brick more.  Nothing in proportion to the frame.
// No global atomics, nothing between workgroups of one launch: ordering comes from the stream.
#define KFX_MESH_UNIT brick_mesh
#include "mesh_cube.h"
#include "mesh_bricks_host.h"

namespace kfx {

// the frame's brick grid as the kernels see it
struct BrickGrid {
    int nbx, nby, nbz;
    unsigned nb;      // bricks of the frame
};

// position of brick `id` in the ascending ids[0, n), -1 if it is not listed (any list: the result is -1 or inside [0, n))
__device__ __forceinline__ int find_brick(const unsigned* __restrict__ ids, unsigned n, unsigned id)
{
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && ids[lo] == id ? (int)lo : -1;
}

// nbr[27 i + k] = the position in to_ids[0, n_to) of neighbour k = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) of brick ids[i], -1 where the
// neighbour lies outside the grid, is not listed, or ids[i] is no brick of the frame.  SELF: to_ids is ids, and brick i is its own k = 13.
template <bool SELF>
__global__ __launch_bounds__(256) void k_bm_neighbours(const BrickGrid g, const unsigned* __restrict__ ids, const unsigned n,
                                                       const unsigned* __restrict__ to_ids, const unsigned n_to, int* __restrict__ nbr)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (unsigned long long)n * BRICK_NEIGHBOURS) return;
    const unsigned i = (unsigned)(t / BRICK_NEIGHBOURS);
    const int k = (int)(t - (unsigned long long)i * BRICK_NEIGHBOURS);
    const unsigned id = ids[i];
    int slot = -1;
    if (id < g.nb) {
        const unsigned bxy = id % ((unsigned)g.nbx * (unsigned)g.nby);
        const int bx = (int)(bxy % (unsigned)g.nbx) + k % 3 - 1, by = (int)(bxy / (unsigned)g.nbx) + (k / 3) % 3 - 1,
                  bz = (int)(id / ((unsigned)g.nbx * (unsigned)g.nby)) + k / 9 - 1;
        if (bx >= 0 && bx < g.nbx && by >= 0 && by < g.nby && bz >= 0 && bz < g.nbz) {
            if (SELF && k == 13) slot = (int)i;
            else slot = find_brick(to_ids, n_to, ((unsigned)bz * (unsigned)g.nby + (unsigned)by) * (unsigned)g.nbx + (unsigned)bx);
        }
    }
    nbr[t] = slot;
}

// Cell (x, y, z) of the frame as a lane sees it whose home brick is (bx0, by0, bz0), position `home` of the list: through the
// home's 27 list positions.  A cell further than one brick from the home, or in an absent brick, reads as `absent`.
template <typename CELL>
struct BrickCells {
    const unsigned char* cells;
    const int* nbr;     // the home brick's 27 positions
    int bx0, by0, bz0;
    float absent;
    __device__ __forceinline__ float operator()(int x, int y, int z) const
    {
        const unsigned dx = (unsigned)((x >> 3) - bx0 + 1), dy = (unsigned)((y >> 3) - by0 + 1), dz = (unsigned)((z >> 3) - bz0 + 1);
        if (dx > 2u || dy > 2u || dz > 2u) return absent;
        const int s = nbr[(dz * 3 + dy) * 3 + dx];
        if (s < 0) return absent;
        return CELL::val(cells + (size_t)s * (BRICK_CELLS * CELL::BYTES), (((z & 7) << 3) | (y & 7)) << 3 | (x & 7));
    }
};

// the first cell of brick id; false if id is no brick of the frame
__device__ __forceinline__ bool brick_origin(const BrickGrid& g, unsigned id, int& x0, int& y0, int& z0)
{
    if (id >= g.nb) return false;
    const unsigned bxy = id % ((unsigned)g.nbx * (unsigned)g.nby);
    x0 = (int)(bxy % (unsigned)g.nbx) * BRICK;
    y0 = (int)(bxy / (unsigned)g.nbx) * BRICK;
    z0 = (int)(id / ((unsigned)g.nbx * (unsigned)g.nby)) * BRICK;
    return true;
}

constexpr int BM_HALO = BRICK + 1, BM_HALO_CELLS = BM_HALO * BM_HALO * BM_HALO;   // 9^3 = 729 corner values of a brick's cubes

// The workgroup's brick (position i of the list, a brick of the frame) as 9^3 corner values in LDS, then the triangle counts of lane
// t's cubes 2 t and 2 t + 1 of the brick in x-major order (local (lx, ly, lz) = (q >> 6, (q >> 3) & 7, q & 7): ascending q is
// ascending dense index); 0 for a cube outside the frame's cubes or with a corner that is not finite.  Plan and emit both classify
// with this, so they agree on which cubes are active.  x0, y0, z0 receive the brick's first cell.
// The loads that depend on nothing but i -- the brick's cells, the neighbour's list position -- are issued before the brick's id is
// looked at (an id that is no brick of the frame has a row of -1 positions, and every count is 0), so that a workgroup waits for two
// rounds of memory, not three.
template <typename CELL>
__device__ __forceinline__ void brick_cube_counts(const MeshParams& p, const unsigned char* __restrict__ cells, const int* __restrict__ nbr27,
                                                  const unsigned i, const unsigned id, const BrickGrid& g, float* lds, unsigned n_tri[2],
                                                  int& x0, int& y0, int& z0)
{
    const int t = (int)threadIdx.x;
    // the brick's own cells: payload cells 2 t, 2 t + 1 (x fastest)
    const float2 own = CELL::pair(cells + (size_t)i * (BRICK_CELLS * CELL::BYTES), 2 * t);
    // the +1 faces, edges and corner, one value per lane t < 217: plane lz = 8 (81 values), then ly = 8 below it (72), then lx = 8 (64)
    int hx = 0, hy = 0, hz = 0, slot = -1;
    const bool halo = t < BM_HALO_CELLS - BRICK_CELLS;
    if (halo) {
        if (t < 81) { hx = t % 9; hy = t / 9; hz = 8; }
        else if (t < 153) { hx = (t - 81) % 9; hy = 8; hz = (t - 81) / 9; }
        else { hx = 8; hy = (t - 153) & 7; hz = (t - 153) >> 3; }
        slot = nbr27[((hz >> 3) + 1) * 9 + ((hy >> 3) + 1) * 3 + (hx >> 3) + 1];
    }
    const bool valid = brick_origin(g, id, x0, y0, z0);
    {
        const int lx = (2 * t) & 7, ly = (t >> 2) & 7, lz = t >> 5;
        lds[(lz * BM_HALO + ly) * BM_HALO + lx] = own.x;
        lds[(lz * BM_HALO + ly) * BM_HALO + lx + 1] = own.y;
    }
    if (halo)
        lds[(hz * BM_HALO + hy) * BM_HALO + hx] =
            slot < 0 ? __builtin_nanf("") : CELL::val(cells + (size_t)slot * (BRICK_CELLS * CELL::BYTES), (((hz & 7) << 3) | (hy & 7)) << 3 | (hx & 7));
    __syncthreads();
    if (!valid) { n_tri[0] = n_tri[1] = 0; return; }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = 2 * t + j, lx = q >> 6, ly = (q >> 3) & 7, lz = q & 7;
        unsigned nt = 0;
        if (x0 + lx < p.cx && y0 + ly < p.cy && z0 + lz < p.cz) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = lds[((lz + corner_dz(c)) * BM_HALO + ly + corner_dy(c)) * BM_HALO + lx + corner_dx(c)];
            int flag;
            if (corner_case(v, flag)) nt = c_num_tris[flag];
        }
        n_tri[j] = nt;
    }
}

__device__ __forceinline__ unsigned bm_pack(unsigned active, unsigned tris) { return (active << 16) | tris; }
__device__ __forceinline__ unsigned bm_active(unsigned c) { return c >> 16; }
__device__ __forceinline__ unsigned bm_tris(unsigned c) { return c & 0xffffu; }

// grid: one workgroup per listed brick; cnt[i] = its active cubes and triangles
template <typename CELL>
__global__ __launch_bounds__(256) void k_bm_count(const MeshParams p, const BrickGrid g, const unsigned* __restrict__ ids,
                                                  const unsigned char* __restrict__ cells, const int* __restrict__ nbr, unsigned* __restrict__ cnt)
{
    __shared__ float lds[BM_HALO_CELLS];
    __shared__ unsigned sums[2][4];
    const unsigned i = blockIdx.x;
    int x0 = 0, y0 = 0, z0 = 0;
    unsigned nt[2];
    brick_cube_counts<CELL>(p, cells, nbr + (size_t)i * BRICK_NEIGHBOURS, i, ids[i], g, lds, nt, x0, y0, z0);   // (an id that is no brick: zeros)
    unsigned a = (nt[0] != 0) + (nt[1] != 0), tr = nt[0] + nt[1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        tr += __shfl_xor(tr, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { sums[0][threadIdx.x >> 6] = a; sums[1][threadIdx.x >> 6] = tr; }
    __syncthreads();
    if (threadIdx.x == 0) cnt[i] = bm_pack(sums[0][0] + sums[0][1] + sums[0][2] + sums[0][3], sums[1][0] + sums[1][1] + sums[1][2] + sums[1][3]);
}

// sums of BRICK_MESH_BLOCK consecutive bricks: part[2 b] = active cubes, part[2 b + 1] = triangles
__global__ __launch_bounds__(256) void k_bm_reduce(const unsigned* __restrict__ cnt, const unsigned n, unsigned* __restrict__ part)
{
    static_assert(BRICK_MESH_BLOCK == 256, "store_block_sums");
    const unsigned i = blockIdx.x * BRICK_MESH_BLOCK + threadIdx.x;
    const unsigned c = i < n ? cnt[i] : 0u;
    store_block_sums(bm_active(c), bm_tris(c), part);
}

// grid: one workgroup per listed brick.  The brick's first cube and triangle = its scan block's offsets + the counts of the bricks
// before it in the block; its active cubes follow in dense order.  Writes stop at the caller's capacities.
template <typename CELL>
__global__ __launch_bounds__(256) void k_bm_compact(const MeshParams p, const BrickGrid g, const unsigned* __restrict__ ids,
                                                    const unsigned char* __restrict__ cells, const int* __restrict__ nbr,
                                                    const unsigned* __restrict__ cnt, const unsigned long long* __restrict__ base,
                                                    long long* __restrict__ cube_index, unsigned* __restrict__ tri_offset,
                                                    const unsigned long long cap_active, const unsigned long long cap_tris)
{
    __shared__ float lds[BM_HALO_CELLS];
    __shared__ unsigned scan[2][4];
    const unsigned i = blockIdx.x;
    if (cnt[i] == 0) return;   // (uniform; also every id that is no brick of the frame)
    int x0 = 0, y0 = 0, z0 = 0;
    const unsigned blk = i / BRICK_MESH_BLOCK, j = blk * BRICK_MESH_BLOCK + threadIdx.x;
    const unsigned before = j < i ? cnt[j] : 0u;
    unsigned before_a, before_t, dummy;
    block_exclusive_scan<unsigned, 4>(bm_active(before), scan[0], &before_a);
    block_exclusive_scan<unsigned, 4>(bm_tris(before), scan[1], &before_t);
    unsigned nt[2];
    brick_cube_counts<CELL>(p, cells, nbr + (size_t)i * BRICK_NEIGHBOURS, i, ids[i], g, lds, nt, x0, y0, z0);
    const unsigned ea = block_exclusive_scan<unsigned, 4>((unsigned)(nt[0] != 0) + (unsigned)(nt[1] != 0), scan[0], &dummy);
    const unsigned et = block_exclusive_scan<unsigned, 4>(nt[0] + nt[1], scan[1], &dummy);
    unsigned long long ia = base[2 * (size_t)blk] + before_a + ea, it = base[2 * (size_t)blk + 1] + before_t + et;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!nt[k]) continue;
        const int q = 2 * (int)threadIdx.x + k;
        const int x = x0 + (q >> 6), y = y0 + ((q >> 3) & 7), z = z0 + (q & 7);
        if (ia < cap_active && it + nt[k] <= cap_tris) {
            cube_index[ia] = ((long long)x * p.cy + y) * p.cz + z;
            tri_offset[ia] = (unsigned)it;
        }
        ++ia;
        it += nt[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Indexed extraction (include/kfx_mesh_bricks_index.h): the brick soup welded by lattice edge into its sequential first-occurrence
// mesh.  As mesh.hip's index, with the soup's order the bricks': the compacted cube list is in that order, so "first in brick-soup
// order" is "lowest list position".  A lattice edge belongs to up to four cubes, in up to four bricks; each is found in two
// dependent steps -- the home brick's 27-neighbour row gives the brick's list position, a binary search in that brick's segment
// [first[b], first[b + 1]) of the cube list gives the cube's -- and the lowest position among those found owns the edge.  (The dense
// rule looks only at the cubes before this one in dense order and stops at the first: here the componentwise-minimum cube may be
// missing and the two diagonal ones are ordered by their bricks.)
//   k_bm_compact           as above, into the index scratch
//   k_bm_first             every listed brick's first cube position (4 bytes)
//   k_mesh_own             mesh_cube.h's, one lane per active cube: case flag and the 12-bit mask of the edges it owns, block sums
//   k_mesh_scan_partials   as above: the blocks' first vertex ids, the vertex total
//   k_mesh_vertex_base     mesh_cube.h's: every active cube's first vertex id (4 bytes)
//   k_mc_emit_indexed      mesh_cube.h's, one lane per active cube: owned edges write their vertex at base + rank; every triangle
//                          corner writes base(owner) + rank(edge in owner)
// Every list position read from the scratches is compared with its list's length before use, and every vertex id with V and face
// slot with the plan's before the store: lists that are not ascending give an unspecified mesh, no access out of bounds.

// first[i] = the position in the compacted cube list of brick i's first cube = its scan block's offset + the active cubes of the
// bricks before it in the block (k_bm_compact's rule)
__global__ __launch_bounds__(256) void k_bm_first(const unsigned* __restrict__ cnt, const unsigned n, const unsigned long long* __restrict__ base,
                                                  unsigned* __restrict__ first)
{
    static_assert(BRICK_MESH_BLOCK == 256, "one brick per thread of the block");
    __shared__ unsigned lds[4];
    const unsigned i = blockIdx.x * BRICK_MESH_BLOCK + threadIdx.x;
    unsigned total;
    const unsigned ex = block_exclusive_scan<unsigned, 4>(i < n ? bm_active(cnt[i]) : 0u, lds, &total);
    if (i < n) first[i] = (unsigned)base[2 * (size_t)blockIdx.x] + ex;
}

// The brick lists as mesh_cube.h's cube source.  A cube's Home is its brick: the position `at` of the list, and the cell accessor
// through that brick's 27-neighbour row.
template <typename CELL>
struct BrickCubes {
    MeshParams p;
    ColorGeom cv;
    int has_color;
    BrickGrid g;
    const unsigned* ids;                // [n], ascending
    unsigned n;
    const unsigned char* cells;
    const int* nbr;                     // [n][27]: k_bm_neighbours<true>'s
    const unsigned char* color_cells;   // an emit's colour list and the SDF bricks' neighbours in it, or null
    const int* cnbr;
    unsigned long long cap_tris;        // the plan's triangle total
    const unsigned* first;              // an index kernel's: [n], every listed brick's first cube in the cube list
    static constexpr bool VERIFIES_LIST = true;
    struct Home {
        int at;
        BrickCells<CELL> sdf;
    };

    // false if ci is no cube of the frame (a negative ci has a negative coordinate)
    __device__ __forceinline__ bool position(long long ci, int& x, int& y, int& z) const
    {
        cube_xyz(p, ci, x, y, z);
        return (unsigned)x < (unsigned)p.cx && (unsigned)y < (unsigned)p.cy && (unsigned)z < (unsigned)p.cz;
    }
    // false if the cube's brick is not listed (a cube of a plan's list has its brick listed)
    __device__ __forceinline__ bool locate(int x, int y, int z, Home& h) const
    {
        const int bx0 = x >> 3, by0 = y >> 3, bz0 = z >> 3;
        h.at = find_brick(ids, n, ((unsigned)bz0 * (unsigned)g.nby + (unsigned)by0) * (unsigned)g.nbx + (unsigned)bx0);
        if (h.at < 0) return false;
        h.sdf = BrickCells<CELL>{cells, nbr + (size_t)h.at * BRICK_NEIGHBOURS, bx0, by0, bz0, __builtin_nanf("")};
        return true;
    }
    __device__ __forceinline__ bool corners(const Home& h, int x, int y, int z, float v[8], int& flag) const
    {
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = h.sdf(x + corner_dx(c), y + corner_dy(c), z + corner_dz(c));
        return corner_case(v, flag);
    }
    // mesh.hip's edge_attributes over the brick lists: multiply-by-reciprocal normalisation, zero where that is not finite
    __device__ __forceinline__ void attributes(const Home& h, const V3& pos, V3& normal, float& grey) const
    {
        const V3 deriv = gradient_over(p, h.sdf, pos);
        V3 nrm = div_s(deriv, length(deriv));
        if (!isfinite(nrm.x) || !isfinite(nrm.y) || !isfinite(nrm.z)) nrm = v3(0.f, 0.f, 0.f);
        normal = nrm;
        grey = 0.f;
        if (has_color && cnbr) {
            const BrickCells<RayC32> col{color_cells, cnbr + (size_t)h.at * BRICK_NEIGHBOURS, h.sdf.bx0, h.sdf.by0, h.sdf.bz0, 0.5f};
            grey = trilinear_over(cv, col, pos);
        } else if (has_color) {   // (no colour bricks at all: every cell reads 0.5)
            grey = trilinear_over(cv, [](int, int, int) { return 0.5f; }, pos);
        }
    }
    // The cube's slots are those the plan counted for it: [tri_offset[t], the next cube's offset or the total).  With ascending ids
    // that is ntri triangles.  With repeated or unsorted ids locate's search may land on another entry than the one the cube was
    // counted from (k_bm_count and k_bm_compact go by list position), and ntri may differ: nothing is written outside the cube's slots.
    __device__ __forceinline__ bool slots(const unsigned* tri_offset, long long t, long long n_active, int, unsigned long long& first_tri,
                                          int& planned) const
    {
        first_tri = tri_offset[t];
        const unsigned long long next = t + 1 < n_active ? (unsigned long long)tri_offset[t + 1] : cap_tris;
        if (next < first_tri || next > cap_tris) return false;
        planned = (int)(next - first_tri);   // (< 2^31: cap_tris < MESH_MAX_TRIS)
        return true;
    }
    // Every other cube around the lattice edge (mesh_cube.h: lattice_edge) that lies in the frame is looked up: its brick is the
    // home's or one of its neighbours (the cube is one cell away), whose list position the home's row holds.
    __device__ __forceinline__ long long owner(const long long* cube_index, long long n_active, long long t, long long ci, int x, int y, int z,
                                               const Home& h, int e, int& oe) const
    {
        const LatticeEdge le = lattice_edge(e);
        const int a = le.a, u = le.u, w = le.w;
        const int at[3] = {x, y, z}, cubes[3] = {p.cx, p.cy, p.cz};
        const long long stride[3] = {(long long)p.cy * p.cz, (long long)p.cz, 1};
        long long best = t;
        oe = e;
#pragma unroll
        for (int su = 0; su < 2; ++su) {
#pragma unroll
            for (int sw = 0; sw < 2; ++sw) {
                const int du = le.m[u] - su, dw = le.m[w] - sw;
                if (du == 0 && dw == 0) continue;   // this cube
                int q[3] = {at[0], at[1], at[2]};
                q[u] += du;
                q[w] += dw;
                if (q[u] < 0 || q[u] >= cubes[u] || q[w] < 0 || q[w] >= cubes[w]) continue;
                const int k = (((q[2] >> 3) - (at[2] >> 3) + 1) * 3 + (q[1] >> 3) - (at[1] >> 3) + 1) * 3 + (q[0] >> 3) - (at[0] >> 3) + 1;
                const int b = h.sdf.nbr[k];
                if (b < 0 || (unsigned)b >= n) continue;   // an absent brick: the cube touches unobserved cells
                // the brick's cubes: [first[b], first[b + 1]) of the list, kept inside it
                long long lo = first[b], hi = (unsigned)b + 1 < n ? (long long)first[b + 1] : n_active;
                if (hi > n_active) hi = n_active;
                const long long want = ci + du * stride[u] + dw * stride[w], end = hi;
                while (lo < hi) {
                    const long long mid = lo + ((hi - lo) >> 1);
                    if (cube_index[mid] < want) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < end && lo < best && cube_index[lo] == want) {
                    best = lo;
                    oe = owner_e(a, su, sw);
                }
            }
        }
        return best;
    }
};

// what every entry point derives from its arguments, after the checks; 0 or the refusal
struct BrickMeshCall {
    BrickGeom geom;
    BrickGrid grid;
    MeshParams p;
    BrickMeshScratch lay;
    int has_color;   // an emit's: colours are asked for and the frame IsValid()
    ColorGeom cv;    // then the colour frame: the SDF frame's dimensions and box
    int* cnbr;       // with colour bricks to read besides: the SDF bricks' neighbours in the colour list (scratch), else null
};

// the sub-buffer at byte offset `off` of a scratch (mesh_bricks_host.h's layouts)
template <typename T>
static T* at(const void* scratch, size_t off) { return (T*)((uintptr_t)scratch + off); }

// The checks of a plan or an emit in one order: the frame and the cell kind, the counts, the lists, the scratch (null, short,
// misaligned), the totals pointer.  `colors`: an emit's colour output, null for a plan.
static int bm_call(BrickMeshCall& c, const char* what, const kfx_volume* frame, int cell, const unsigned* ids, const void* cells, unsigned long long n,
                   const unsigned* color_ids, const void* color_cells, unsigned long long n_color, const void* scratch, size_t scratch_bytes,
                   const unsigned long long* totals, const float* colors = nullptr)
{
    if (int e = refuse(brick_check_frame(frame, cell, c.geom), what)) return e;
    if (int e = refuse(brick_check_counts(n, n_color), what)) return e;
    if (int e = refuse(brick_check_lists(ids, cells, n), what)) return e;
    if (int e = refuse(brick_check_lists(color_ids, color_cells, n_color), what)) return e;
    if (int e = refuse(brick_mesh_check_scratch(n, n_color, scratch, scratch_bytes), what)) return e;
    if (!totals) return fail_rule(what, KFX_E_NULL, "null totals");
    c.grid = BrickGrid{c.geom.nbx, c.geom.nby, c.geom.nbz, (unsigned)c.geom.nb};
    // the frame's geometry as the dense extractor's mesh_setup fills it (no storage behind it: ptr and pitches are not the frame's)
    kfx_volume f = *frame;
    f.ptr = nullptr;
    f.pitch = f.img_pitch = 0;
    set_geometry(c.p, &f);
    set_voxel_size(c.p, &f);
    c.p.cx = (int)f.w - 1; c.p.cy = (int)f.h - 1; c.p.cz = (int)f.d - 1;
    c.p.avail_lo = 0;
    c.p.avail_hi = (int)f.d;
    c.lay = brick_mesh_scratch(n, n_color);
    c.has_color = brick_mesh_has_color(c.geom, colors) ? 1 : 0;
    c.cv = ColorGeom{};
    if (c.has_color) set_geometry(c.cv, &f);
    c.cnbr = c.has_color && n_color ? at<int>(scratch, c.lay.cnbr) : nullptr;
    return 0;
}

// the lists of a call as the kernels' cube source; `first`: an index kernel's (index scratch), else null
template <typename CELL>
static BrickCubes<CELL> brick_cubes(const BrickMeshCall& c, const unsigned* ids, unsigned long long n, const void* cells, const void* color_cells,
                                    const void* scratch, const unsigned long long* totals, const unsigned* first)
{
    return {c.p, c.cv, c.has_color, c.grid, ids, (unsigned)n, (const unsigned char*)cells, at<const int>(scratch, c.lay.nbr),
            (const unsigned char*)color_cells, c.cnbr, totals[1], first};
}

// an emit's first launch, with colour bricks to read: the SDF bricks' neighbours in the colour list
static void launch_color_neighbours(const BrickMeshCall& c, const unsigned* ids, unsigned long long n, const unsigned* color_ids,
                                    unsigned long long n_color, hipStream_t st)
{
    if (c.cnbr)
        hipLaunchKernelGGL(k_bm_neighbours<false>, dim3((unsigned)((n * BRICK_NEIGHBOURS + 255) / 256)), dim3(256), 0, st, c.grid, ids, (unsigned)n,
                           color_ids, (unsigned)n_color, c.cnbr);
}

template <typename F>
static void for_sdf_cell(int cell, F f)
{
    if (cell == KFX_CELL_F32) f(RayF32{});
    else f(RayF16{});
}

// k_bm_compact of a planned scratch into an emit's or an index plan's lists
template <typename CELL>
static void launch_compact(const BrickMeshCall& c, const unsigned* ids, unsigned long long n, const void* cells, const void* scratch,
                           const unsigned long long* totals, long long* cube_index, unsigned* tri_offset, hipStream_t st)
{
    hipLaunchKernelGGL(k_bm_compact<CELL>, dim3((unsigned)n), dim3(256), 0, st, c.p, c.grid, ids, (const unsigned char*)cells,
                       at<const int>(scratch, c.lay.nbr), at<const unsigned>(scratch, c.lay.cnt), at<const unsigned long long>(scratch, c.lay.base),
                       cube_index, tri_offset, totals[0], totals[1]);
}

} // namespace kfx

using namespace kfx;

extern "C" size_t kfx_mesh_bricks_scratch_bytes(unsigned long long n, unsigned long long n_color)
{
    if (brick_check_counts(n, n_color).code) return 0;
    return brick_mesh_scratch(n, n_color).bytes;
}

extern "C" int kfx_mesh_bricks_plan(const kfx_volume* frame, int cell, const unsigned* ids, const void* cells, unsigned long long n, void* scratch,
                                    size_t scratch_bytes, unsigned long long totals[2], kfx_stream stream)
{
    const char* const what = "kfx_mesh_bricks_plan";
    BrickMeshCall c;
    if (int e = bm_call(c, what, frame, cell, ids, cells, n, nullptr, nullptr, 0, scratch, scratch_bytes, totals)) return e;
    totals[0] = totals[1] = 0;
    if (n == 0) return 0;
    if (int e = load_tables()) return e;
    int* const nbr = at<int>(scratch, c.lay.nbr);
    unsigned* const cnt = at<unsigned>(scratch, c.lay.cnt);
    unsigned* const part = at<unsigned>(scratch, c.lay.part);
    unsigned long long* const hdr = at<unsigned long long>(scratch, c.lay.hdr);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nn = (unsigned)n;
    hipLaunchKernelGGL(k_bm_neighbours<true>, dim3((unsigned)((n * BRICK_NEIGHBOURS + 255) / 256)), dim3(256), 0, st, c.grid, ids, nn, ids, nn, nbr);
    for_sdf_cell(cell, [&](auto kind) {
        using CELL = decltype(kind);
        hipLaunchKernelGGL(k_bm_count<CELL>, dim3(nn), dim3(256), 0, st, c.p, c.grid, ids, (const unsigned char*)cells, (const int*)nbr, cnt);
    });
    hipLaunchKernelGGL(k_bm_reduce, dim3((unsigned)c.lay.nblk), dim3(256), 0, st, (const unsigned*)cnt, nn, part);
    hipLaunchKernelGGL(k_mesh_scan_partials, dim3(1), dim3(MESH_SCAN_THREADS), 0, st, (const unsigned*)part, (long long)c.lay.nblk,
                       at<unsigned long long>(scratch, c.lay.base), hdr);
    if (int e = check_launch(what)) return e;
    unsigned long long host[2];
    if (int e = read_header(host, hdr, 2, st)) return e;
    totals[0] = host[0];
    totals[1] = host[1];
    if (totals[1] >= MESH_MAX_TRIS) return fail_rule(what, KFX_E_RANGE, "2^32/3 triangles or more (32-bit vertex offsets)");
    return 0;
}

extern "C" int kfx_mesh_bricks_emit(const kfx_volume* frame, int cell, const unsigned* ids, const void* cells, unsigned long long n,
                                    const unsigned* color_ids, const void* color_cells, unsigned long long n_color, void* scratch,
                                    size_t scratch_bytes, const unsigned long long totals[2], long long* cube_index, unsigned* tri_offset,
                                    float* verts, float* norms, float* colors, kfx_stream stream)
{
    const char* const what = "kfx_mesh_bricks_emit";
    BrickMeshCall c;
    if (int e = bm_call(c, what, frame, cell, ids, cells, n, color_ids, color_cells, n_color, scratch, scratch_bytes, totals, colors)) return e;
    if (!totals_in_range(totals)) return fail_rule(what, KFX_E_RANGE, "totals out of range");
    if (n == 0) return totals[0] || totals[1] ? fail_rule(what, KFX_E_RANGE, "totals are not the plan's") : 0;
    if (totals[0] == 0) return 0;
    if (int e = refuse(brick_mesh_check_outputs(cube_index, tri_offset, verts, norms, colors), what)) return e;
    if (int e = load_tables()) return e;
    const hipStream_t st = (hipStream_t)stream;
    if (int e = check_planned(at<const unsigned long long>(scratch, c.lay.hdr), totals, 2, what, st)) return e;
    const long long n_active = (long long)totals[0];
    launch_color_neighbours(c, ids, n, color_ids, n_color, st);
    for_sdf_cell(cell, [&](auto kind) {
        using CELL = decltype(kind);
        launch_compact<CELL>(c, ids, n, cells, scratch, totals, cube_index, tri_offset, st);
        hipLaunchKernelGGL(k_mc_emit<BrickCubes<CELL>>, dim3((unsigned)((n_active + 127) / 128)), dim3(128), 0, st,
                           brick_cubes<CELL>(c, ids, n, cells, color_cells, scratch, totals, nullptr), (const long long*)cube_index,
                           (const unsigned*)tri_offset, n_active, verts, norms, c.has_color ? colors : nullptr);
    });
    return check_launch(what);
}

// ---- indexed extraction (include/kfx_mesh_bricks_index.h) ----

static_assert(BRICK_MESH_MAX_TRIS == MESH_MAX_TRIS && BRICK_MESH_IDX_BLOCK == MESH_IDX_BLOCK, "mesh_bricks_host.h states mesh_cube.h's limits");

// The checks of an index plan or an indexed emit after bm_call's, in one order: the totals (null, range, with V), then the index
// scratch (null, short, misaligned); the carved index scratch in x.
static int bm_index_call(BrickMeshIndexScratch& x, const char* what, unsigned long long n, const unsigned long long* totals, unsigned long long n_verts,
                         const void* index_scratch, size_t index_scratch_bytes)
{
    if (int e = refuse(brick_mesh_check_totals(totals, n_verts), what)) return e;
    if (int e = refuse(brick_mesh_index_check_scratch(n, totals, index_scratch, index_scratch_bytes), what)) return e;
    x = brick_mesh_index_scratch(n, totals[0]);
    return 0;
}

extern "C" size_t kfx_mesh_bricks_index_scratch_bytes(unsigned long long n, const unsigned long long totals[2])
{
    if (brick_check_counts(n, 0).code || brick_mesh_check_totals(totals, 0).code) return 0;
    return brick_mesh_index_scratch(n, totals[0]).bytes;
}

extern "C" int kfx_mesh_bricks_index_plan(const kfx_volume* frame, int cell, const unsigned* ids, const void* cells, unsigned long long n,
                                          const void* scratch, size_t scratch_bytes, const unsigned long long totals[2], void* index_scratch,
                                          size_t index_scratch_bytes, unsigned long long* n_verts, kfx_stream stream)
{
    const char* const what = "kfx_mesh_bricks_index_plan";
    BrickMeshCall c;
    BrickMeshIndexScratch x;
    if (int e = bm_call(c, what, frame, cell, ids, cells, n, nullptr, nullptr, 0, scratch, scratch_bytes, totals)) return e;
    if (int e = bm_index_call(x, what, n, totals, 0, index_scratch, index_scratch_bytes)) return e;
    if (!n_verts) return fail_rule(what, KFX_E_NULL, "null n_verts");
    if (n == 0 && (totals[0] || totals[1])) return fail_rule(what, KFX_E_RANGE, "totals are not the plan's");
    *n_verts = 0;
    if (n == 0 || totals[0] == 0) return 0;
    if (int e = load_tables()) return e;
    unsigned long long* const xhdr = at<unsigned long long>(index_scratch, x.hdr);
    long long* const cube_index = at<long long>(index_scratch, x.cube_index);
    unsigned* const tri_offset = at<unsigned>(index_scratch, x.tri_offset);
    unsigned* const info = at<unsigned>(index_scratch, x.info);
    unsigned* const first = at<unsigned>(index_scratch, x.first);
    unsigned* const xpart = at<unsigned>(index_scratch, x.part);
    unsigned long long* const xbase = at<unsigned long long>(index_scratch, x.base);
    const hipStream_t st = (hipStream_t)stream;
    if (int e = check_planned(at<const unsigned long long>(scratch, c.lay.hdr), totals, 2, what, st)) return e;
    const long long n_active = (long long)totals[0];
    for_sdf_cell(cell, [&](auto kind) {
        using CELL = decltype(kind);
        launch_compact<CELL>(c, ids, n, cells, scratch, totals, cube_index, tri_offset, st);
        hipLaunchKernelGGL(k_bm_first, dim3((unsigned)c.lay.nblk), dim3(256), 0, st, at<const unsigned>(scratch, c.lay.cnt), (unsigned)n,
                           at<const unsigned long long>(scratch, c.lay.base), first);
        hipLaunchKernelGGL(k_mesh_own<BrickCubes<CELL>>, dim3((unsigned)x.nblk), dim3(MESH_IDX_BLOCK), 0, st,
                           brick_cubes<CELL>(c, ids, n, cells, nullptr, scratch, totals, first), (const long long*)cube_index,
                           (const unsigned*)tri_offset, n_active, totals[1], info, xpart, xhdr);
        hipLaunchKernelGGL(k_mesh_scan_partials, dim3(1), dim3(MESH_SCAN_THREADS), 0, st, (const unsigned*)xpart, (long long)x.nblk, xbase, xhdr);
        hipLaunchKernelGGL(k_mesh_vertex_base, dim3((unsigned)x.nblk), dim3(MESH_IDX_BLOCK), 0, st, (const unsigned*)info, n_active,
                           (const unsigned long long*)xbase, at<unsigned>(index_scratch, x.vbase));
    });
    if (int e = check_launch(what)) return e;
    unsigned long long host[2];
    if (int e = read_header(host, xhdr, 2, st)) return e;
    *n_verts = host[0];
    return 0;
}

extern "C" int kfx_mesh_bricks_emit_indexed(const kfx_volume* frame, int cell, const unsigned* ids, const void* cells, unsigned long long n,
                                            const unsigned* color_ids, const void* color_cells, unsigned long long n_color, void* scratch,
                                            size_t scratch_bytes, const void* index_scratch, size_t index_scratch_bytes,
                                            const unsigned long long totals[2], unsigned long long n_verts, float* verts, float* norms,
                                            float* colors, unsigned* faces, kfx_stream stream)
{
    const char* const what = "kfx_mesh_bricks_emit_indexed";
    BrickMeshCall c;
    BrickMeshIndexScratch x;
    if (int e = bm_call(c, what, frame, cell, ids, cells, n, color_ids, color_cells, n_color, scratch, scratch_bytes, totals, colors)) return e;
    if (int e = bm_index_call(x, what, n, totals, n_verts, index_scratch, index_scratch_bytes)) return e;
    if (n == 0) return totals[0] || totals[1] || n_verts ? fail_rule(what, KFX_E_RANGE, "totals are not the plan's") : 0;
    if (totals[0] == 0) return 0;
    if (int e = refuse(brick_mesh_check_indexed_outputs(verts, norms, colors, faces), what)) return e;
    if (int e = load_tables()) return e;
    const hipStream_t st = (hipStream_t)stream;
    // (the index plan's header: vertices, triangles, and the totals it was planned for)
    const unsigned long long planned[4] = {n_verts, totals[1], totals[0], totals[1]};
    if (int e = check_planned(at<const unsigned long long>(index_scratch, x.hdr), planned, 4, what, st)) return e;
    const long long n_active = (long long)totals[0];
    launch_color_neighbours(c, ids, n, color_ids, n_color, st);
    for_sdf_cell(cell, [&](auto kind) {
        using CELL = decltype(kind);
        hipLaunchKernelGGL(k_mc_emit_indexed<BrickCubes<CELL>>, dim3((unsigned)((n_active + 127) / 128)), dim3(128), 0, st,
                           brick_cubes<CELL>(c, ids, n, cells, color_cells, scratch, totals, at<const unsigned>(index_scratch, x.first)),
                           at<const long long>(index_scratch, x.cube_index), at<const unsigned>(index_scratch, x.tri_offset),
                           at<const unsigned>(index_scratch, x.info), at<const unsigned>(index_scratch, x.vbase), n_active, n_verts, verts, norms,
                           c.has_color ? colors : nullptr, faces);
    });
    return check_launch(what);
}
