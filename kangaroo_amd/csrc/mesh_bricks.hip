// mesh_bricks.hip -- marching cubes straight from packed 8 x 8 x 8 bricks (include/kfx_mesh_bricks.h): the mesh of a FRAME, a virtual
// dense volume of which only the listed bricks exist and every other cell is NaN (colour: 0.5), without that volume.  The result is
// the dense extractor's (mesh.hip) on the volume the bricks would unpack into, bit for bit: a cube's case, a vertex's position, the
// normalisation and the store are mesh_cube.h's, shared with it; the frame's geometry is a MeshParams filled by the same set_geometry;
// the gradient stencil and the colour blend are sampling.h's own (gradient_over, trilinear_over: the dense samplers' base cell and blend)
// over a cell accessor that goes through the brick lists.
//
//   k_bm_neighbours   one lane per (listed brick, neighbour): the neighbour's position in the ascending id list by binary search, -1
//                     if absent -- 27 positions per brick, the brick's own among them.  After this a frame cell within 8 cells of a
//                     brick is two dependent loads away.  The same kernel maps the SDF list's neighbours into the colour list.
//   k_bm_count        one workgroup per listed brick: its 9 x 9 x 9 corner values in LDS (2916 bytes) -- its own 8^3 by one 16- / 8-byte
//                     load per lane, the +1 faces, edges and corner from up to seven neighbours -- then two cubes per lane, those
//                     inside the frame's (w - 1, h - 1, d - 1); active cubes and triangles of the brick, 4 bytes.
//   k_bm_reduce, k_bm_scan   sums of 256 bricks, their exclusive offsets and the totals (mesh_cube.h's scan)
//   k_bm_compact      one workgroup per listed brick with cubes: stages and classifies again, ranks its active cubes in dense order
//                     (lane t holds cubes 2 t, 2 t + 1 of the brick in x-major order = ascending ci) and writes cube_index / tri_offset
//   k_bm_emit         one lane per ACTIVE cube, as k_mc_emit: the cube's brick by binary search, corners and stencils through the
//                     neighbour table
// Memory: the lists, about 112 (colour: 220) bytes of scratch per listed brick, the outputs.  Nothing in proportion to the frame.
// No global atomics, nothing between workgroups of one launch: ordering comes from the stream.
#include "mesh_cube.h"
#include "mesh_bricks_host.h"

namespace kfx {

__constant__ unsigned char c_bm_num_tris[256];
__constant__ unsigned short c_bm_edge_mask[256];
__constant__ signed char c_bm_tris[256][15];

static bool g_bm_tables_loaded[64] = {};
static int bm_load_tables()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (g_bm_tables_loaded[dev]) return 0;
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_bm_num_tris), MC_NUM_TRIS, sizeof(MC_NUM_TRIS));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_bm_edge_mask), MC_EDGE_MASK, sizeof(MC_EDGE_MASK));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_bm_tris), MC_TRIS, sizeof(MC_TRIS));
    if (e != hipSuccess) return set_error((int)e, hipGetErrorString(e));
    g_bm_tables_loaded[dev] = true;
    return 0;
}

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
            if (corner_case(v, flag)) nt = c_bm_num_tris[flag];
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

__global__ __launch_bounds__(MESH_SCAN_THREADS) void k_bm_scan(const unsigned* __restrict__ part, const long long nblk,
                                                               unsigned long long* __restrict__ base, unsigned long long* __restrict__ totals)
{
    scan_block_sums(part, nblk, base, totals);
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

// k_mc_emit over bricks: one thread per active cube, the same steps and expressions
template <typename CELL>
__global__ __launch_bounds__(128) void k_bm_emit(const MeshParams p, const ColorGeom cv, const int has_color, const BrickGrid g,
                                                 const unsigned* __restrict__ ids, const unsigned n, const unsigned char* __restrict__ cells,
                                                 const int* __restrict__ nbr, const unsigned char* __restrict__ color_cells,
                                                 const int* __restrict__ cnbr, const long long* __restrict__ cube_index,
                                                 const unsigned* __restrict__ tri_offset, const long long n_active,
                                                 const unsigned long long cap_tris, float* __restrict__ verts, float* __restrict__ norms,
                                                 float* __restrict__ colors)
{
    const long long t_id = (long long)blockIdx.x * 128 + threadIdx.x;
    if (t_id >= n_active) return;
    int x, y, z, flag;
    cube_xyz(p, cube_index[t_id], x, y, z);
    if ((unsigned)x >= (unsigned)p.cx || (unsigned)y >= (unsigned)p.cy || (unsigned)z >= (unsigned)p.cz) return;
    const int bx0 = x >> 3, by0 = y >> 3, bz0 = z >> 3;
    const int home = find_brick(ids, n, ((unsigned)bz0 * (unsigned)g.nby + (unsigned)by0) * (unsigned)g.nbx + (unsigned)bx0);
    if (home < 0) return;   // (a cube of a plan's list has its brick listed)
    const BrickCells<CELL> sdf{cells, nbr + (size_t)home * BRICK_NEIGHBOURS, bx0, by0, bz0, __builtin_nanf("")};
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = sdf(x + corner_dx(c), y + corner_dy(c), z + corner_dz(c));
    if (!corner_case(v, flag)) return;
    const int ntri = c_bm_num_tris[flag];
    if (ntri == 0) return;
    const unsigned mask = c_bm_edge_mask[flag];
    const V3 p0 = cube_origin(p, x, y, z);
    V3 ev[12], en[12];
    float ec[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        if (!(mask & (1u << e))) continue;
        ev[e] = edge_position(p, p0, v, e);
        // (mesh.hip's edge_attributes: multiply-by-reciprocal normalisation, zero where that is not finite)
        const V3 deriv = gradient_over(p, sdf, ev[e]);
        V3 nrm = div_s(deriv, length(deriv));
        if (!isfinite(nrm.x) || !isfinite(nrm.y) || !isfinite(nrm.z)) nrm = v3(0.f, 0.f, 0.f);
        en[e] = nrm;
        ec[e] = 0.f;
        if (has_color && cnbr) {
            const BrickCells<RayC32> grey{color_cells, cnbr + (size_t)home * BRICK_NEIGHBOURS, bx0, by0, bz0, 0.5f};
            ec[e] = trilinear_over(cv, grey, ev[e]);
        } else if (has_color) {   // (no colour bricks at all: every cell reads 0.5)
            ec[e] = trilinear_over(cv, [](int, int, int) { return 0.5f; }, ev[e]);
        }
    }
    // The cube's slots are those the plan counted for it: [tri_offset[t_id], the next cube's offset or the total).  With ascending ids
    // that is ntri triangles.  With repeated or unsorted ids the search above may land on another entry than the one the cube was
    // counted from (k_bm_count and k_bm_compact go by list position), and ntri may differ: nothing is written outside the cube's slots.
    const unsigned long long first = tri_offset[t_id], next = t_id + 1 < n_active ? (unsigned long long)tri_offset[t_id + 1] : cap_tris;
    if (next < first || next > cap_tris) return;
    const int planned = (int)(next - first < 5 ? next - first : 5);
    size_t o = (size_t)first * 3; // first output vertex of this cube
    for (int t = 0; t < min(ntri, planned) * 3; ++t, ++o) {
        const int e = c_bm_tris[flag][t];
        V3 P = v3(0.f, 0.f, 0.f), N = P;
        float C = 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k)   // select without dynamic register indexing
            if (k == e) { P = ev[k]; N = en[k]; C = ec[k]; }
        store_vertex(verts, norms, colors, o, P, N, C, has_color);
    }
}

// what every entry point derives from its arguments, after the checks; 0 or the refusal
struct BrickMeshCall {
    BrickGeom geom;
    BrickGrid grid;
    MeshParams p;
    BrickMeshScratch lay;
};

// The checks of a plan or an emit in one order: the frame and the cell kind, the counts, the lists, the scratch (null, short,
// misaligned), the totals pointer.
static int bm_call(BrickMeshCall& c, const char* what, const kfx_volume* frame, int cell, const unsigned* ids, const void* cells, unsigned long long n,
                   const unsigned* color_ids, const void* color_cells, unsigned long long n_color, const void* scratch, size_t scratch_bytes,
                   const unsigned long long* totals)
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
    return 0;
}

template <typename F>
static void for_sdf_cell(int cell, F f)
{
    if (cell == KFX_CELL_F32) f(RayF32{});
    else f(RayF16{});
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
    if (int e = bm_load_tables()) return e;
    unsigned char* const s = (unsigned char*)scratch;
    int* const nbr = (int*)(s + c.lay.nbr);
    unsigned* const cnt = (unsigned*)(s + c.lay.cnt);
    unsigned* const part = (unsigned*)(s + c.lay.part);
    unsigned long long* const base = (unsigned long long*)(s + c.lay.base);
    unsigned long long* const hdr = (unsigned long long*)(s + c.lay.hdr);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned nn = (unsigned)n;
    hipLaunchKernelGGL(k_bm_neighbours<true>, dim3((unsigned)((n * BRICK_NEIGHBOURS + 255) / 256)), dim3(256), 0, st, c.grid, ids, nn, ids, nn, nbr);
    for_sdf_cell(cell, [&](auto kind) {
        using CELL = decltype(kind);
        hipLaunchKernelGGL(k_bm_count<CELL>, dim3(nn), dim3(256), 0, st, c.p, c.grid, ids, (const unsigned char*)cells, (const int*)nbr, cnt);
    });
    hipLaunchKernelGGL(k_bm_reduce, dim3((unsigned)c.lay.nblk), dim3(256), 0, st, (const unsigned*)cnt, nn, part);
    hipLaunchKernelGGL(k_bm_scan, dim3(1), dim3(MESH_SCAN_THREADS), 0, st, (const unsigned*)part, (long long)c.lay.nblk, base, hdr);
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
    if (int e = bm_call(c, what, frame, cell, ids, cells, n, color_ids, color_cells, n_color, scratch, scratch_bytes, totals)) return e;
    if (!totals_in_range(totals)) return fail_rule(what, KFX_E_RANGE, "totals out of range");
    if (n == 0) return totals[0] || totals[1] ? fail_rule(what, KFX_E_RANGE, "totals are not the plan's") : 0;
    if (totals[0] == 0) return 0;
    if (int e = refuse(brick_mesh_check_outputs(cube_index, tri_offset, verts, norms, colors), what)) return e;
    const int has_color = brick_mesh_has_color(c.geom, colors) ? 1 : 0;
    ColorGeom cv{};
    if (has_color) {   // the colour frame: the SDF frame's dimensions and box
        kfx_volume f = *frame;
        f.ptr = nullptr;
        f.pitch = f.img_pitch = 0;
        set_geometry(cv, &f);
    }
    if (int e = bm_load_tables()) return e;
    unsigned char* const s = (unsigned char*)scratch;
    const int* const nbr = (const int*)(s + c.lay.nbr);
    const unsigned* const cnt = (const unsigned*)(s + c.lay.cnt);
    const unsigned long long* const base = (const unsigned long long*)(s + c.lay.base);
    int* const cnbr = has_color && n_color ? (int*)(s + c.lay.cnbr) : nullptr;
    const hipStream_t st = (hipStream_t)stream;
    if (int e = check_planned((const unsigned long long*)(s + c.lay.hdr), totals, 2, what, st)) return e;
    const unsigned nn = (unsigned)n;
    const long long n_active = (long long)totals[0];
    if (cnbr)
        hipLaunchKernelGGL(k_bm_neighbours<false>, dim3((unsigned)((n * BRICK_NEIGHBOURS + 255) / 256)), dim3(256), 0, st, c.grid, ids, nn, color_ids,
                           (unsigned)n_color, cnbr);
    for_sdf_cell(cell, [&](auto kind) {
        using CELL = decltype(kind);
        hipLaunchKernelGGL(k_bm_compact<CELL>, dim3(nn), dim3(256), 0, st, c.p, c.grid, ids, (const unsigned char*)cells, nbr, cnt, base, cube_index,
                           tri_offset, totals[0], totals[1]);
        hipLaunchKernelGGL(k_bm_emit<CELL>, dim3((unsigned)((n_active + 127) / 128)), dim3(128), 0, st, c.p, cv, has_color, c.grid, ids, nn,
                           (const unsigned char*)cells, nbr, (const unsigned char*)color_cells, (const int*)cnbr, (const long long*)cube_index,
                           (const unsigned*)tri_offset, n_active, totals[1], verts, norms, has_color ? colors : nullptr);
    });
    return check_launch(what);
}
