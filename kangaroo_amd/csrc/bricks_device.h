// bricks_device.h -- the kernels bricks.hip (include/kfx_bricks.h) and brick_pool.hip (include/kfx_brick_pool.h) share: which bricks of
// a view are live, the scan of a flag byte per entry into ascending ids, and the move of a brick between a view and 512 packed cells.
//
//   k_brick_flags          one streaming read of the view, organised by volume rows: a workgroup owns a run of 1 KiB of
//                          cells along x (16 bricks of SDF_t, 32 of the 4-byte cells) in one (by, bz) -- 64 rows -- and each wave
//                          sweeps 16 of those rows, a lane one 16-byte segment of the address space (one load where the segment lies
//                          inside the run, cell by cell at a run's unaligned head and tail).  Words are compared with the fill's;
//                          a lane keeps what it found per brick in two registers (a segment meets two bricks at the most), ORs
//                          them into the workgroup's LDS flags once, and the workgroup writes one flag byte per brick it owns.
//   k_brick_count          flagged entries per scan block of 256 entries (ballot + popcount)
//   k_brick_scan_partials  one wave: exclusive offsets of the scan blocks, and the total
//   k_brick_ids            the flagged entries at the scanned offsets
//   brick_move_lane        pack / unpack: 16 bytes of the payload per lane (fully coalesced: a brick is 4 or 2 KiB, one or half a
//                          workgroup), the volume side 16 bytes where the row segment is aligned and inside the view, cell by cell
//                          otherwise; unpack writes cells inside the view only.
// No global atomics, nothing between workgroups of one launch: ordering comes from the stream.  The kernels that are no templates
// have internal linkage: each translation unit that includes this launches its own.
#pragma once

#include <cstring>
#include <type_traits>

#include "kfx_device.h"
#include "host_args.h"
#include "block_scan.h"
#include "bricks_host.h"

namespace kfx {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

template <int CELL> struct BrickCell;
template <> struct BrickCell<4> { typedef unsigned T; };
template <> struct BrickCell<8> { typedef unsigned long long T; };

struct BrickArgs {
    unsigned char* vol;          // cell (0, 0, 0) of the view
    size_t pitch, img;
    int w, h, d;
    int nbx, nby;
    unsigned nb;                 // bricks of the view
    unsigned long long fill;     // the fill cell's bytes (CELL 4: the low word)
    int aligned;                 // every row of the view starts on a 16-byte boundary
};

template <int CELL>
__device__ __forceinline__ void cells_of(const v4u v, typename BrickCell<CELL>::T* c)
{
    if constexpr (CELL == 4) { c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w; }
    else { c[0] = (unsigned long long)v.x | ((unsigned long long)v.y << 32); c[1] = (unsigned long long)v.z | ((unsigned long long)v.w << 32); }
}
template <int CELL>
__device__ __forceinline__ v4u vector_of(const typename BrickCell<CELL>::T* c)
{
    v4u v;
    if constexpr (CELL == 4) { v.x = c[0]; v.y = c[1]; v.z = c[2]; v.w = c[3]; }
    else { v.x = (unsigned)c[0]; v.y = (unsigned)(c[0] >> 32); v.z = (unsigned)c[1]; v.w = (unsigned)(c[1] >> 32); }
    return v;
}

// grid (runs along x, nby, nbz); flags[id] = 1 where brick id holds a cell that is not the fill's bytes, else 0
template <int CELL>
__global__ __launch_bounds__(256) void k_brick_flags(const BrickArgs a, unsigned char* __restrict__ flags)
{
    typedef typename BrickCell<CELL>::T cell_t;
    constexpr int CPS = 16 / CELL;      // cells per 16-byte segment
    constexpr int RUN = 1024 / CELL;    // cells of a run
    constexpr int BPR = RUN / BRICK;    // bricks of a run
    __shared__ unsigned live[BPR];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const cell_t fill = (cell_t)a.fill;
    if (threadIdx.x < BPR) live[threadIdx.x] = 0;
    __syncthreads();
    const int xr0 = (int)blockIdx.x * RUN;                            // the run: cells [xr0, xr0 + n) of the rows
    const int n = a.w - xr0 < RUN ? a.w - xr0 : RUN;
    const int y0 = (int)blockIdx.y * BRICK, z0 = (int)blockIdx.z * BRICK;
    // A row's first cell lies mis cells (0 .. CPS - 1) beyond a 16-byte boundary, and segment s of the row holds the run's cells
    // s * CPS - mis + k: up to 65 segments where mis != 0, so a second pass serves segment 64 (lane 0 alone; skipped where every
    // row is aligned).  Whatever mis is, segment s meets the bricks bl and bh of the run only.
    for (int s = lane; s < (a.aligned ? 64 : 128); s += 64) {
        const int bl = (s * CPS - CPS + 1) >> 3, bh = (s * CPS + CPS - 1) >> 3;
        bool dl = false, dh = false;
#pragma unroll 4
        for (int r = wave; r < BRICK * BRICK; r += 4) {
            const int y = y0 + (r & 7), z = z0 + (r >> 3);
            if (y >= a.h || z >= a.d) continue;
            const unsigned char* const row = a.vol + (size_t)z * a.img + (size_t)y * a.pitch + (size_t)xr0 * CELL;
            const int mis = (int)(((uintptr_t)row & 15) / CELL);
            const int c0 = s * CPS - mis;                              // the segment's first cell, counted from the run's
            if (c0 >= n) continue;
            cell_t c[CPS];
            if (c0 >= 0 && c0 + CPS <= n) {
                cells_of<CELL>(__builtin_nontemporal_load(reinterpret_cast<const v4u*>(row + (ptrdiff_t)c0 * CELL)), c);
            } else {
#pragma unroll
                for (int k = 0; k < CPS; ++k)
                    c[k] = (unsigned)(c0 + k) < (unsigned)n ? __builtin_nontemporal_load(reinterpret_cast<const cell_t*>(row) + (c0 + k)) : fill;
            }
#pragma unroll
            for (int k = 0; k < CPS; ++k) {
                const bool differs = c[k] != fill, low = ((c0 + k) >> 3) == bl;
                dl |= differs && low;
                dh |= differs && !low;
            }
        }
        // (a set bit stands for a cell inside the run, so its brick is one of the run's: 0 <= bl, bh < BPR)
        if (dl) live[bl] = 1;
        if (dh) live[bh] = 1;
    }
    __syncthreads();
    const int bx = (int)blockIdx.x * BPR + (int)threadIdx.x;
    if (threadIdx.x < BPR && bx < a.nbx)
        flags[((size_t)blockIdx.z * a.nby + blockIdx.y) * a.nbx + bx] = (unsigned char)live[threadIdx.x];
}

// part[b] = live bricks among the BRICK_SCAN_BLOCK bricks of scan block b
static __global__ __launch_bounds__(256) void k_brick_count(const unsigned char* __restrict__ flags, const unsigned nb, unsigned* __restrict__ part)
{
    __shared__ unsigned sums[4];
    const unsigned id = blockIdx.x * BRICK_SCAN_BLOCK + threadIdx.x;
    const unsigned long long m = __ballot(id < nb && flags[id] != 0);
    if ((threadIdx.x & 63) == 0) sums[threadIdx.x >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = sums[0] + sums[1] + sums[2] + sums[3];
}

// one wave: base[b] = live bricks before scan block b, *total = all of them
static __global__ __launch_bounds__(64) void k_brick_scan_partials(const unsigned* __restrict__ part, const unsigned nblk, unsigned* __restrict__ base,
                                                                   unsigned long long* __restrict__ total)
{
    const unsigned lane = threadIdx.x;
    unsigned run = 0;
    for (unsigned b0 = 0; b0 < nblk; b0 += 64) {
        const unsigned b = b0 + lane;
        const unsigned v = b < nblk ? part[b] : 0u;
        unsigned inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(inc, o, 64);
            if (lane >= (unsigned)o) inc += t;
        }
        if (b < nblk) base[b] = run + inc - v;
        run += __shfl(inc, 63, 64);
    }
    if (lane == 0) *total = run;
}

// ids[k] = the k-th live brick; nothing at or beyond ids[n_live]
static __global__ __launch_bounds__(256) void k_brick_ids(const unsigned char* __restrict__ flags, const unsigned nb, const unsigned* __restrict__ base,
                                                          const unsigned n_live, unsigned* __restrict__ ids)
{
    __shared__ unsigned lds[4];
    const unsigned id = blockIdx.x * BRICK_SCAN_BLOCK + threadIdx.x;
    const unsigned f = id < nb && flags[id] != 0 ? 1u : 0u;
    unsigned total;
    const unsigned k = block_exclusive_scan<unsigned, 4>(f, lds, &total) + base[blockIdx.x];
    if (f && k < n_live) ids[k] = id;
}

// Brick id of the view <-> brick[8][8][8], 512 packed cells.  Lane t of the brick's 256 (SDF_t) or 128 lanes owns 16 bytes of the
// payload: CPS cells of one brick row.  UNPACK = false reads the view (the fill's bytes outside it) and writes the payload;
// UNPACK = true reads the payload and writes the cells inside the view.  An id >= the brick count is skipped.
template <int CELL, bool UNPACK>
__device__ __forceinline__ void brick_move_lane(const BrickArgs& a, const unsigned id, unsigned char* brick, const int t)
{
    typedef typename BrickCell<CELL>::T cell_t;
    constexpr int CPS = 16 / CELL;
    constexpr int SPR = BRICK / CPS;                  // segments per brick row
    if (id >= a.nb) return;
    const unsigned bxy = id % ((unsigned)a.nbx * (unsigned)a.nby);
    const int x = (int)(bxy % (unsigned)a.nbx) * BRICK + (t % SPR) * CPS;
    const int y = (int)(bxy / (unsigned)a.nbx) * BRICK + ((t / SPR) & 7);
    const int z = (int)(id / ((unsigned)a.nbx * (unsigned)a.nby)) * BRICK + t / (SPR * BRICK);
    v4u* const payload = reinterpret_cast<v4u*>(brick + (size_t)t * 16);
    const bool row_in = y < a.h && z < a.d && x < a.w;
    unsigned char* const p = a.vol + (row_in ? (size_t)z * a.img + (size_t)y * a.pitch + (size_t)x * CELL : 0);
    const bool whole = row_in && x + CPS <= a.w && ((uintptr_t)p & 15) == 0;
    cell_t c[CPS];
    if constexpr (!UNPACK) {
        const cell_t fill = (cell_t)a.fill;
#pragma unroll
        for (int k = 0; k < CPS; ++k) c[k] = fill;
        if (whole) {
            cells_of<CELL>(__builtin_nontemporal_load(reinterpret_cast<const v4u*>(p)), c);
        } else if (row_in) {
#pragma unroll
            for (int k = 0; k < CPS; ++k)
                if (x + k < a.w) c[k] = __builtin_nontemporal_load(reinterpret_cast<const cell_t*>(p) + k);
        }
        __builtin_nontemporal_store(vector_of<CELL>(c), payload);
    } else {
        const v4u v = __builtin_nontemporal_load(payload);
        if (whole) {
            *reinterpret_cast<v4u*>(p) = v;
        } else if (row_in) {
            cells_of<CELL>(v, c);
#pragma unroll
            for (int k = 0; k < CPS; ++k)
                if (x + k < a.w) reinterpret_cast<cell_t*>(p)[k] = c[k];
        }
    }
}

// lanes per brick, bricks per workgroup of 256
template <int CELL> struct BrickLanes {
    static constexpr int TPB = BRICK_CELLS * CELL / 16;
    static constexpr unsigned PER_GROUP = 256 / TPB;
};

// what every entry point derives from a view, after the checks; 0 or the refusal
struct BrickSetup {
    BrickGeom g;
    size_t cb;
    BrickArgs a;
};
inline int brick_setup(BrickSetup& s, const kfx_volume* vol, int cell, float fill, const char* what)
{
    if (!vol || !vol->ptr) return fail_rule(what, KFX_E_NULL, "null volume");
    s.cb = shift_cell_bytes(cell);
    if (!s.cb) return fail_rule(what, KFX_E_RANGE, "unknown cell kind");
    if (int e = check_volume(vol, s.cb, 1, VOLUME_MAX_DIM, what)) return e;
    s.g = brick_geom(vol->w, vol->h, vol->d);
    if (int e = refuse(brick_check_grid(s.g), what)) return e;
    s.a = BrickArgs{(unsigned char*)vol->ptr, vol->pitch, vol->img_pitch, s.g.w, s.g.h, s.g.d, s.g.nbx, s.g.nby, (unsigned)s.g.nb,
                    shift_fill_bytes(cell, fill), (((uintptr_t)vol->ptr | vol->pitch | vol->img_pitch) & 15) == 0 ? 1 : 0};
    return 0;
}

template <typename F>
inline void for_cell_bytes(size_t cb, F f)
{
    if (cb == 8) f(std::integral_constant<int, 8>());
    else f(std::integral_constant<int, 4>());
}

// the classification and the scan of a view's bricks, enqueued: flags, per-block counts and offsets, the total in *total
static inline void launch_brick_flags(const BrickSetup& s, unsigned char* flags, hipStream_t st)
{
    for_cell_bytes(s.cb, [&](auto cb) {
        constexpr int CELL = decltype(cb)::value;
        const dim3 grid((unsigned)ceil_div(s.g.w, 1024 / CELL), (unsigned)s.g.nby, (unsigned)s.g.nbz);
        hipLaunchKernelGGL(k_brick_flags<CELL>, grid, dim3(256), 0, st, s.a, flags);
    });
}
static inline void launch_brick_scan(const unsigned char* flags, unsigned n, unsigned nblk, unsigned* part, unsigned* base, unsigned long long* total, hipStream_t st)
{
    hipLaunchKernelGGL(k_brick_count, dim3(nblk), dim3(256), 0, st, flags, n, part);
    hipLaunchKernelGGL(k_brick_scan_partials, dim3(1), dim3(64), 0, st, (const unsigned*)part, nblk, base, total);
}

} // namespace kfx
