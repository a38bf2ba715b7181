// summary.hip -- the brick summary of a TSDF volume (kfx_sdf_summary, include/kfx.h): creation, the conservative state
// changes for writers that do not track (invalidate), SdfReset with tracking, and the class tables R -> C the ray-march
// stages in LDS.  The summary is maintained by k_sdf_fuse_tiled<..., TRACK> (fuse.hip) and consumed by
// k_raycast_sdf_classes (raycast.hip).  No reference counterpart: the reference's march samples the volume at every step (cu_raycast.cu:58-81).
#include <algorithm>
#include <new>

#include <hip/hip_fp16.h>

#include "kfx_device.h"

namespace kfx {

__global__ __launch_bounds__(256) void k_summary_fill(float4* __restrict__ R, size_t n, float lo, float hi, int state)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) R[i] = make_float4(lo, hi, __int_as_float(state), 0.f);
}

// Class tables (ClassView, kfx_device.h).  One lane per entry, 64 consecutive entries of a row per wave; the two planes are
// the wave's ballots.
//   fine level (2^shift cells, shift 3 or 4): from the summary bricks [b << (shift - 3), (b + 1) << (shift - 3)] per axis
//   (the last one holds the +1 cells), clamped to the grid;
//   32^3-cell level: the cells [32 c, 32 c + 32] of entry c are exactly those of the fine entries [c m, c m + m) per axis
//   (m = 32 >> shift; each fine entry already includes its +1 cells), i.e. of the bricks [4 c, 4 c + 4], and a class is an AND
//   over bricks: the same bits either from the 125 brick ranges (M = 4) or from m^3 two-bit reads of the fine level's words
//   (M = 0, `src`).  LDS mode: from R, by further workgroups of the launch that builds the fine level -- no workgroup reads
//   what another one of the launch writes, so one launch per build does (k_summary_classes_build).  Global-table mode (built on
//   every call, tables of ~2000^3 volumes): from the fine level's words, in a launch of its own behind the fine level's.
// The workgroups of the 32^3-cell level add up their entries of class != 0; the last workgroup to arrive publishes the total
// with the build's stamp in host-visible memory (*publish) and clears the counters for the next build -- the host reads that
// slot without synchronising (raycast.hip, class_view; summary_ring_host.h).
struct ClassBuild {
    const float4* R;
    unsigned* C;
    int nbx, nby, nbz;
    int shift, nx, ny, nz, rw;
    float lo_ok, hi_ok;
    const unsigned* src;   // M == 0: the fine level's words
    int src_shift, src_nx, src_ny, src_nz, src_rw;
};
// The 64^3- and 128^3-cell levels (LDS mode; the global-table mode builds them with launches of their own): derived from the
// 32^3-cell level by the last workgroup of its build, into the words summary_top_layout assigns behind it.  tab: the tables' first word.
struct TopBuild {
    int on;
    unsigned* tab;
    ClassLevel l5, l6, l7;
    int nx5, nz5, nx6, nz6, nx7, nz7;
};
// one wave = 64 consecutive entries of a row; returns (lane 0) the number of them with class != 0
template <int M>   // summary bricks per fine entry and axis (1: 8^3 cells, 2: 16^3, 4: 32^3 straight from R); 0: combine `src`
__device__ __forceinline__ int class_row(const ClassBuild& b, const long long wave)
{
    const float4* __restrict__ R = b.R;
    unsigned* __restrict__ C = b.C;
    const unsigned* __restrict__ src = b.src;
    const int nbx = b.nbx, nby = b.nby, nbz = b.nbz, shift = b.shift, nx = b.nx, ny = b.ny, rw = b.rw;
    const int src_shift = b.src_shift, src_nx = b.src_nx, src_ny = b.src_ny, src_nz = b.src_nz, src_rw = b.src_rw;
    const float lo_ok = b.lo_ok, hi_ok = b.hi_ok;
    const int lane = threadIdx.x & 63;
    const int chunks = (nx + 63) >> 6;
    const int chunk = (int)(wave % chunks), by = (int)((wave / chunks) % ny), bz = (int)(wave / ((long long)chunks * ny));
    const int bx = chunk * 64 + lane;
    int cls = 0;
    if (bx < nx) {
        bool all_nan = true, all_free = true, all_either = true;
        if constexpr (M == 0) {
            const int m = 1 << (shift - src_shift);   // 2 (16^3-cell fine level) or 4 (8^3)
            // the m entries along x lie in one word pair (m divides 32): one 8-byte read per (y, z), all requested up front
            for (int z0 = 0; z0 < m; z0 += 2) {
                uint2 w2[2][4];
#pragma unroll
                for (int dz = 0; dz < 2; ++dz)
#pragma unroll
                    for (int dy = 0; dy < 4; ++dy) {
                        const int z = min(bz * m + z0 + dz, src_nz - 1), y = min(by * m + min(dy, m - 1), src_ny - 1);
                        w2[dz][dy] = *reinterpret_cast<const uint2*>(src + ((size_t)z * src_ny + y) * src_rw + (((bx * m) >> 5) << 1));
                    }
#pragma unroll
                for (int dz = 0; dz < 2; ++dz)
#pragma unroll
                    for (int dy = 0; dy < 4; ++dy)
                        for (int dx = 0; dx < m; ++dx) {
                            const int x = min(bx * m + dx, src_nx - 1);   // (clamped entries repeat a neighbour: same verdict)
                            const int c = (int)((w2[dz][dy].x >> (x & 31)) & 1u) | (int)(((w2[dz][dy].y >> (x & 31)) & 1u) << 1);
                            all_free = all_free && c == 1;
                            all_nan = all_nan && c == 2;
                            all_either = all_either && c != 0;
                        }
            }
        } else if constexpr (M > 2) {
            // 125 ranges per entry: loops over z and y (kept loops: unrolled, or with a plane's 25 ranges requested together, the
            // build kernel spills 16-34 SGPRs and its no-fine-level variant takes scratch), the five ranges of a row along x
            // requested together
#pragma unroll 1
            for (int z = bz * M; z <= bz * M + M; ++z)
#pragma unroll 1
                for (int y = by * M; y <= by * M + M; ++y) {
                    const float4* __restrict__ Rrow = R + ((size_t)min(z, nbz - 1) * nby + min(y, nby - 1)) * nbx;
                    float4 r[M + 1];
#pragma unroll
                    for (int dx = 0; dx <= M; ++dx) r[dx] = Rrow[min(bx * M + dx, nbx - 1)];
#pragma unroll
                    for (int dx = 0; dx <= M; ++dx) {
                        const unsigned m = brick_class_mask(r[dx].x, r[dx].y, __float_as_int(r[dx].z), lo_ok, hi_ok);
                        all_nan = all_nan && (m & 1u);
                        all_free = all_free && (m & 2u);
                        all_either = all_either && (m & 4u);
                    }
                }
        } else {
            // (M + 1)^3 brick ranges, all requested before the first is looked at (fully unrolled: the loop form waited for
            // each row of loads in turn, 9.5 us per launch at 512^3 against ~3)
            float4 r[(M + 1) * (M + 1) * (M + 1)];
#pragma unroll
            for (int dz = 0; dz <= M; ++dz)
#pragma unroll
                for (int dy = 0; dy <= M; ++dy)
#pragma unroll
                    for (int dx = 0; dx <= M; ++dx)
                        r[(dz * (M + 1) + dy) * (M + 1) + dx] =
                            R[((size_t)min(bz * M + dz, nbz - 1) * nby + min(by * M + dy, nby - 1)) * nbx + min(bx * M + dx, nbx - 1)];
#pragma unroll
            for (int k = 0; k < (M + 1) * (M + 1) * (M + 1); ++k) {
                const unsigned m = brick_class_mask(r[k].x, r[k].y, __float_as_int(r[k].z), lo_ok, hi_ok);
                all_nan = all_nan && (m & 1u);
                all_free = all_free && (m & 2u);
                all_either = all_either && (m & 4u);
            }
        }
        cls = all_free ? 1 : (all_nan ? 2 : (all_either ? 3 : 0));
    }
    const unsigned long long p0 = __ballot(cls & 1), p1 = __ballot(cls & 2);
    if (lane == 0) {
        unsigned* row = C + ((size_t)bz * ny + by) * rw + chunk * 4;
        row[0] = (unsigned)p0; row[1] = (unsigned)p1;
        if (chunk * 4 + 2 < rw) { row[2] = (unsigned)(p0 >> 32); row[3] = (unsigned)(p1 >> 32); }
    }
    return __popcll(p0 | p1);
}

// What the workgroups of a build's counting launch do first (conditional: the host knows of nothing but tracked SdfFuse launches
// since the last build): the tables are rebuilt only if one of those launches saw a brick change its class mask (*dirty,
// kfx_sdf_summary::d_dirty); otherwise they are the bits this launch would write, nothing is built, and one thread publishes
// the retained total under this build's stamp, so the host sees what it would have seen.  Every workgroup reads *dirty before
// any other work; true: leave.
__device__ __forceinline__ bool classes_up_to_date(int* __restrict__ count, unsigned long long* __restrict__ publish, const unsigned stamp,
                                                   const int* __restrict__ dirty, const int conditional)
{
    if (!conditional || *dirty != 0) return false;   // (uniform)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        __hip_atomic_store(publish, ((unsigned long long)stamp << 32) | (unsigned)count[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        count[4] += 1;
    }
    return true;
}

// ... and last.  n: this wave's entries of the 32^3-cell level with class != 0 (lane 0; 0 for a wave that built fine rows).  The
// workgroups add theirs up (LDS), take a ticket, and the last of ALL the launch's workgroups publishes the total with the
// build's stamp in one 64-bit store to host-visible memory and clears the counters for the next build.  count = {running total,
// tickets taken, the total of the last real build, conditional builds that built, conditional builds that returned early}.  The
// last workgroup retains the total and clears *dirty: every workgroup of the launch -- of both levels: a ticket over the
// 32^3-cell level's alone would let a fine workgroup dispatched late read the cleared word and leave stale rows -- has read it
// by then.  It also derives the two coarser levels (TopBuild) from rows that other workgroups -- on other XCDs, whose L2s are
// not coherent with this one's -- wrote: the writers' agent-scope fence before the ticket and this workgroup's agent-scope
// fence after it order those rows before the reads.
__device__ __forceinline__ void classes_count_and_top(const int n, int* __restrict__ count, unsigned long long* __restrict__ publish, const unsigned stamp,
                                                      int* __restrict__ dirty, const int conditional, const TopBuild& t)
{
    __shared__ int s_count[4];
    __shared__ int s_last;
    if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = n;
    __threadfence();   // (release, agent scope: this thread's rows, for the workgroup that derives the coarser levels)
    __syncthreads();
    if (threadIdx.x == 0) {
        s_last = 0;
        atomicAdd(&count[0], s_count[0] + s_count[1] + s_count[2] + s_count[3]);
        __threadfence();
        if (atomicAdd(&count[1], 1) == (int)gridDim.x - 1) {   // every workgroup's contribution is in
            __threadfence();
            s_last = 1;
            const int total = atomicExch(&count[0], 0);
            count[1] = 0;
            count[2] = total;
            if (conditional) count[3] += 1;
            *dirty = 0;
            __hip_atomic_store(publish, ((unsigned long long)stamp << 32) | (unsigned)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    __syncthreads();
    if (t.on && s_last) {   // (uniform) the last workgroup: every row of the 32^3-cell level has been written and released
        __threadfence();    // (acquire, agent scope, by every thread that is about to read them)
        classes_level_up(t.tab, t.l5, t.nx5, t.nz5, t.l6, t.nx6, t.nz6);
        __threadfence();
        __syncthreads();
        classes_level_up(t.tab, t.l6, t.nx6, t.nz6, t.l7, t.nx7, t.nz7);
    }
}

// LDS mode, one launch per build: workgroups [0, f.blocks) write the fine level's rows (MF = 1: 8^3 cells, 2: 16^3, 0: no fine
// level, f.blocks = 0), the others the 32^3-cell level's (c) straight from R.  No workgroup waits for another.
struct FineRows {   // what the fine level's ClassBuild differs in from the 32^3-cell level's
    unsigned* C;
    int shift, nx, ny, nz, rw;
    int blocks;
    long long waves;
};
template <int MF>
__global__ __launch_bounds__(256) void k_summary_classes_build(const FineRows f, const ClassBuild c, const long long c_waves, int* __restrict__ count,
                                                               unsigned long long* __restrict__ publish, const unsigned stamp, int* __restrict__ dirty,
                                                               const int conditional, const TopBuild t)
{
    if (classes_up_to_date(count, publish, stamp, dirty, conditional)) return;
    int n = 0;
    bool fine_row = false;
    if constexpr (MF != 0) {
        fine_row = (int)blockIdx.x < f.blocks;   // (uniform)
        if (fine_row) {
            ClassBuild b = c;
            b.C = f.C; b.shift = f.shift; b.nx = f.nx; b.ny = f.ny; b.nz = f.nz; b.rw = f.rw;
            const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
            if (wave < f.waves) class_row<MF>(b, wave);
        }
    }
    if (!fine_row) {
        const long long wave = (long long)((int)blockIdx.x - f.blocks) * 4 + (threadIdx.x >> 6);
        if (wave < c_waves) n = class_row<4>(c, wave);
    }
    classes_count_and_top(n, count, publish, stamp, dirty, conditional, t);
}

// Global-table mode: a level in a launch of its own, one wave per row of 64 entries (M = 1, 2: the fine level; 0: the 64^3- and
// 128^3-cell levels, each from the level below it) ...
template <int M>
__global__ __launch_bounds__(256) void k_summary_classes(const ClassBuild b, const long long n_waves)
{
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wave < n_waves) class_row<M>(b, wave);
}

// ... and the 32^3-cell level from the fine level's words, with the count (never conditional: this mode builds on every call)
__global__ __launch_bounds__(256) void k_summary_classes_coarse(const ClassBuild b, const long long n_waves, int* __restrict__ count,
                                                                unsigned long long* __restrict__ publish, const unsigned stamp, int* __restrict__ dirty, const TopBuild t)
{
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n = wave < n_waves ? class_row<0>(b, wave) : 0;
    classes_count_and_top(n, count, publish, stamp, dirty, 0, t);
}

// kfx_sdf_summary_rebuild: R from the volume itself.  One wave per 8 x 8 x 8 brick: a lane reads one row of eight cells (four
// 16-byte loads: 64 contiguous bytes), keeps the range of the values and whether it saw a NaN / a value; DPP and permlane swaps
// reduce the wave.  The states are the TRACK kernels' (kfx_device.h): 0 every cell valued, 1 every cell NaN, 2 both kinds --
// with the exact range of the valued cells in every case, which is at least as tight as what tracking arrives at.
// BYTES = 4 (SDF_h cells): a lane's row of eight half cells is 32 contiguous bytes, two 16-byte loads of {val, w} pairs; the
// range is kept in fp32, where every half value is exact.
template <int BYTES>
__global__ __launch_bounds__(256) void k_summary_rebuild(float4* __restrict__ R, const unsigned char* __restrict__ base, size_t pitch, size_t img_pitch,
                                                         int w, int h, int d, int nbx, int nby, int nbz, int aligned16)
{
    const long long brick = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (brick >= (long long)nbx * nby * nbz) return;   // wave-uniform
    const int lane = threadIdx.x & 63;
    const int bx = (int)(brick % nbx), by = (int)((brick / nbx) % nby), bz = (int)(brick / ((long long)nbx * nby));
    const int y = by * 8 + (lane & 7), z = bz * 8 + (lane >> 3), x0 = bx * 8;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    bool nan = false, val = false;
    if (y < h && z < d) {
        const unsigned char* row = base + (size_t)z * img_pitch + (size_t)y * pitch + (size_t)x0 * BYTES;
        if (BYTES == 4 && x0 + 8 <= w && aligned16) {
            uint4 c[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) c[k] = reinterpret_cast<const uint4*>(row)[k];   // {cell, cell, cell, cell}, half {val, w} each
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const unsigned u[4] = {c[k].x, c[k].y, c[k].z, c[k].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float a = __half2float(__ushort_as_half((unsigned short)(u[j] & 0xffffu)));
                    nan = nan || a != a;
                    val = val || a == a;
                    lo = fminf(lo, a);
                    hi = fmaxf(hi, a);
                }
            }
        } else if (BYTES == 8 && x0 + 8 <= w && aligned16) {
            float4 c[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = reinterpret_cast<const float4*>(row)[k];   // {val, w, val, w}
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = c[k].x, b = c[k].z;
                nan = nan || a != a || b != b;
                val = val || a == a || b == b;
                lo = fminf(lo, fminf(a, b));   // (minNum / maxNum: a NaN operand leaves the other)
                hi = fmaxf(hi, fmaxf(a, b));
            }
        } else {
            const int x1 = x0 + 8 < w ? x0 + 8 : w;   // this brick's eight cells (fewer in the volume's last brick)
            for (int x = x0; x < x1; ++x) {
                const float a = BYTES == 8 ? *reinterpret_cast<const float*>(row + (size_t)(x - x0) * 8)
                                           : __half2float(__ushort_as_half(*reinterpret_cast<const unsigned short*>(row + (size_t)(x - x0) * 4)));
                nan = nan || a != a;
                val = val || a == a;
                lo = fminf(lo, a);
                hi = fmaxf(hi, a);
            }
        }
    }
    const auto fmin2 = [](float a, float b) { return fminf(a, b); };
    const auto fmax2 = [](float a, float b) { return fmaxf(a, b); };
    lo = wave_xor_combine<1>(lo, fmin2); hi = wave_xor_combine<1>(hi, fmax2);
    lo = wave_xor_combine<2>(lo, fmin2); hi = wave_xor_combine<2>(hi, fmax2);
#pragma unroll
    for (int off = 4; off <= 8; off <<= 1) { lo = fminf(lo, __shfl_xor(lo, off, 64)); hi = fmaxf(hi, __shfl_xor(hi, off, 64)); }
    lo = wave_xor_combine<16>(lo, fmin2); hi = wave_xor_combine<16>(hi, fmax2);
    lo = wave_xor_combine<32>(lo, fmin2); hi = wave_xor_combine<32>(hi, fmax2);
    const bool any_nan = __ballot(nan) != 0ull, any_val = __ballot(val) != 0ull;
    if (lane == 0) R[brick] = make_float4(lo, hi, __int_as_float(any_val ? (any_nan ? 2 : 0) : 1), 0.f);
}

static void class_level(ClassLevel& L, int shift, int w, int h, int first)
{
    L.shift = shift;
    L.ny = ceil_div(h, 1 << shift);
    L.rw = 2 * ceil_div(ceil_div(w, 1 << shift), 32);
    L.first = first;
}
static int class_level_words(const ClassLevel& L, int d) { return L.rw * L.ny * ceil_div(d, 1 << L.shift); }

// layout of the tables for a fine level of 2^fine_shift cells (3 or 4; 5 = the coarse level only)
void summary_class_layout(const kfx_sdf_summary* s, int fine_shift, ClassView& cv)
{
    class_level(cv.fine, fine_shift, s->w, s->h, 0);
    const int fw = fine_shift < 5 ? class_level_words(cv.fine, s->d) : 0;
    class_level(cv.coarse, 5, s->w, s->h, (fw + 3) & ~3);
    cv.words = cv.coarse.first + ((class_level_words(cv.coarse, s->d) + 3) & ~3);
}

void summary_top_layout(const ClassView& cv, ClassLevel& l6, ClassLevel& l7, int& w6, int& w7)
{
    int nx6, nz6, nx7, nz7;
    class_level_up(cv.nx5, cv.coarse.ny, cv.nz5, 6, cv.words, l6, nx6, nz6, w6);
    class_level_up(nx6, l6.ny, nz6, 7, cv.words + w6, l7, nx7, nz7, w7);
}

int summary_classes_prepare(kfx_sdf_summary* s, float tol, float vref, int fine_shift, hipStream_t stream, int global)
{
    const bool same = s->c_tol == tol && s->c_vref == vref && s->c_shift == fine_shift && s->c_global == global;
    if (!s->c_dirty && same) return 0;
    // Only tracked SdfFuse launches since the tables were built for these parameters: the same launch, which returns at once
    // unless one of those saw a brick change its class mask (d_dirty).  Everything else -- and the global-table mode, whose
    // levels are built by launches of their own and which the headline does not run -- builds unconditionally.
    const int conditional = (s->c_dirty == 1 && same && !global) ? 1 : 0;
    ClassView cv;
    summary_class_layout(s, fine_shift, cv);
    cv.nx5 = ceil_div(s->w, 32); cv.nz5 = ceil_div(s->d, 32);
    ClassLevel l6, l7;
    int w6, w7;
    summary_top_layout(cv, l6, l7, w6, w7);
    TopBuild top{};
    top.on = global ? 0 : 1;
    top.tab = s->C;
    top.l5 = cv.coarse; top.l6 = l6; top.l7 = l7;
    top.nx5 = cv.nx5; top.nz5 = cv.nz5;
    top.nx6 = (top.nx5 + 1) >> 1; top.nz6 = (top.nz5 + 1) >> 1;
    top.nx7 = (top.nx6 + 1) >> 1; top.nz7 = (top.nz6 + 1) >> 1;
    const float lo_ok = vref - tol * vref, hi_ok = vref + tol * vref;
    // the rows of level L: from R, or (src) from the words of the level below it
    auto level = [&](const ClassLevel& L, const ClassLevel* src) {
        const ClassLevel& S = src ? *src : L;
        ClassBuild b;
        b.R = s->R; b.C = s->C + L.first;
        b.nbx = s->nbx; b.nby = s->nby; b.nbz = s->nbz;
        b.shift = L.shift; b.nx = ceil_div(s->w, 1 << L.shift); b.ny = L.ny; b.nz = ceil_div(s->d, 1 << L.shift); b.rw = L.rw;
        b.lo_ok = lo_ok; b.hi_ok = hi_ok;
        b.src = src ? s->C + S.first : nullptr;
        b.src_shift = S.shift; b.src_nx = ceil_div(s->w, 1 << S.shift); b.src_ny = S.ny; b.src_nz = ceil_div(s->d, 1 << S.shift); b.src_rw = S.rw;
        return b;
    };
    auto waves_of = [](const ClassBuild& b) { return (long long)ceil_div(b.nx, 64) * b.ny * b.nz; };
    auto blocks_of = [&](const ClassBuild& b) { return (unsigned)((waves_of(b) + 3) / 4); };
    auto launched = [&]() { s->launches += 1; return check_launch("kfx_sdf_summary (classes)"); };
    const bool has_fine = fine_shift < 5;
    // build number s->builds: its stamp, and its slot of the ring (without pinned memory: a device word nobody reads)
    const unsigned stamp = summary_ring_stamp(s->builds);
    unsigned long long* publish = s->d_skippable + (s->h_skippable ? summary_ring_index(s->builds) : 0);
    if (global && has_fine) {
        // global-table mode: the fine level, then the 32^3-cell level from its words with the count
        const ClassBuild f = level(cv.fine, nullptr), c = level(cv.coarse, &cv.fine);
        if (cv.fine.shift == 3) hipLaunchKernelGGL(k_summary_classes<1>, dim3(blocks_of(f)), dim3(256), 0, stream, f, waves_of(f));
        else hipLaunchKernelGGL(k_summary_classes<2>, dim3(blocks_of(f)), dim3(256), 0, stream, f, waves_of(f));
        if (int e = launched()) return e;
        hipLaunchKernelGGL(k_summary_classes_coarse, dim3(blocks_of(c)), dim3(256), 0, stream, c, waves_of(c), s->d_count, publish, stamp, s->d_dirty, top);
        if (int e = launched()) return e;
    } else {
        // one launch: the fine level's workgroups (none where the 32^3-cell level is the finest), then the 32^3-cell level's
        const ClassBuild c = level(cv.coarse, nullptr);
        FineRows f{};
        if (has_fine) {
            const ClassBuild b = level(cv.fine, nullptr);
            f.C = b.C; f.shift = b.shift; f.nx = b.nx; f.ny = b.ny; f.nz = b.nz; f.rw = b.rw;
            f.blocks = (int)blocks_of(b); f.waves = waves_of(b);
        }
        const dim3 grid((unsigned)f.blocks + blocks_of(c));
        if (!has_fine) hipLaunchKernelGGL(k_summary_classes_build<0>, grid, dim3(256), 0, stream, f, c, waves_of(c), s->d_count, publish, stamp, s->d_dirty, conditional, top);
        else if (cv.fine.shift == 3) hipLaunchKernelGGL(k_summary_classes_build<1>, grid, dim3(256), 0, stream, f, c, waves_of(c), s->d_count, publish, stamp, s->d_dirty, conditional, top);
        else hipLaunchKernelGGL(k_summary_classes_build<2>, grid, dim3(256), 0, stream, f, c, waves_of(c), s->d_count, publish, stamp, s->d_dirty, conditional, top);
        if (int e = launched()) return e;
    }
    s->builds += 1;
    if (global) {
        // global-table mode: the 64^3- and 128^3-cell levels, each the combination of the level below it (m = 2) -- the same
        // entries classes_level_up derives in the LDS mode's build
        for (int up = 0; up < 2; ++up) {
            const ClassBuild b = level(up ? l7 : l6, up ? &l6 : &cv.coarse);
            hipLaunchKernelGGL(k_summary_classes<0>, dim3(blocks_of(b)), dim3(256), 0, stream, b, waves_of(b));
            if (int e = launched()) return e;
        }
    }
    s->c_dirty = 0; s->c_tol = tol; s->c_vref = vref; s->c_shift = fine_shift; s->c_global = global;
    s->c_lo_ok = lo_ok; s->c_hi_ok = hi_ok;
    return 0;
}

int summary_view_offset(const kfx_sdf_summary* s, const kfx_volume* view, int* ox, int* oy, int* oz)
{
    if (!s || !view || !view->ptr) return set_error(KFX_E_NULL, "summary: null argument");
    if (view->pitch != s->pitch || view->img_pitch != s->img_pitch) return set_error(KFX_E_SHAPE, "summary: the volume is not a view of the summary's volume (pitches)");
    const unsigned char* q = static_cast<const unsigned char*>(view->ptr);
    if (q < s->base) return set_error(KFX_E_SHAPE, "summary: the volume is not a view of the summary's volume");
    const size_t off = (size_t)(q - s->base);
    const size_t z = off / s->img_pitch, rem = off % s->img_pitch, y = rem / s->pitch, xb = rem % s->pitch;
    const size_t cb = (size_t)s->cell_bytes;
    if (xb % cb || z + view->d > (size_t)s->d || y + view->h > (size_t)s->h || xb / cb + view->w > (size_t)s->w)
        return set_error(KFX_E_SHAPE, "summary: the volume is not a view of the summary's volume (extent)");
    *ox = (int)(xb / cb); *oy = (int)y; *oz = (int)z;
    return 0;
}

} // namespace kfx

using namespace kfx;

static int summary_create(kfx_sdf_summary** out, const kfx_volume* vol, int cell_bytes)
{
    if (!out || !vol || !vol->ptr) return set_error(KFX_E_NULL, "kfx_sdf_summary_create: null argument");
    if (vol->w < 2 || vol->h < 2 || vol->d < 2 || vol->w > 65535 || vol->h > 65535 || vol->d > 65535) return set_error(KFX_E_SHAPE, "kfx_sdf_summary_create: volume dimensions");
    kfx_sdf_summary* s = new (std::nothrow) kfx_sdf_summary;
    if (!s) return set_error(KFX_E_RANGE, "kfx_sdf_summary_create: out of memory");
    s->nbx = ceil_div((int)vol->w, 8); s->nby = ceil_div((int)vol->h, 8); s->nbz = ceil_div((int)vol->d, 8);
    s->w = (int)vol->w; s->h = (int)vol->h; s->d = (int)vol->d;
    s->cell_bytes = cell_bytes;
    s->base = static_cast<const unsigned char*>(vol->ptr);
    s->pitch = vol->pitch; s->img_pitch = vol->img_pitch;
    s->R = nullptr; s->C = nullptr; s->d_count = nullptr; s->h_skippable = nullptr; s->d_skippable = nullptr;
    s->c_dirty = 2; s->c_tol = -1.f; s->c_vref = 0.f; s->c_shift = 0; s->c_global = 0; s->sweeps = 0;
    s->keep_stride = 0; s->keep_row0 = 0; s->keep_rows = 0;
    s->c_lo_ok = 0.f; s->c_hi_ok = 0.f; s->d_dirty = nullptr;
    s->builds = 0; s->plain_calls = 0; s->launches = 0;
    s->n_coarse = ceil_div(s->w, 32) * ceil_div(s->h, 32) * ceil_div(s->d, 32);
    const size_t n = (size_t)s->nbx * s->nby * s->nbz;
    ClassView cv;
    summary_class_layout(s, 3, cv);   // the finest level is the largest table; behind it, the 64^3- and 128^3-cell levels
    cv.nx5 = ceil_div(s->w, 32); cv.nz5 = ceil_div(s->d, 32);
    ClassLevel l6, l7;
    int w6, w7;
    summary_top_layout(cv, l6, l7, w6, w7);   // (the two levels' sizes do not depend on the fine level)
    const int words = cv.words + w6 + w7;
    bool ok = hipMalloc((void**)&s->R, n * sizeof(float4)) == hipSuccess && hipMalloc((void**)&s->C, (size_t)words * sizeof(unsigned)) == hipSuccess &&
              hipMalloc((void**)&s->d_count, 64 * sizeof(int)) == hipSuccess && hipMemset(s->d_count, 0, 64 * sizeof(int)) == hipSuccess;
    if (ok) s->d_dirty = s->d_count + 32;   // (a cache line of its own: the kernels that set it store plainly, the counters are atomics)
    // the published counts live in pinned host memory the device can write (mapped: coherent, a system-scope store is seen by
    // the host while the stream runs on); without it the march always uses the tables.  Slots start unstamped (zero).
    if (ok && hipHostMalloc((void**)&s->h_skippable, KFX_SUMMARY_RING * sizeof(unsigned long long), hipHostMallocMapped) == hipSuccess) {
        for (int i = 0; i < KFX_SUMMARY_RING; ++i) s->h_skippable[i] = 0ull;
        if (hipHostGetDevicePointer((void**)&s->d_skippable, s->h_skippable, 0) != hipSuccess) {
            (void)hipHostFree(s->h_skippable);
            s->h_skippable = nullptr;
        }
    } else {
        s->h_skippable = nullptr;
    }
    if (ok && !s->h_skippable) {   // a device word nobody reads keeps the kernel's interface the same
        (void)hipGetLastError();
        ok = hipMalloc((void**)&s->d_skippable, sizeof(unsigned long long)) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        kfx_sdf_summary_destroy(s);
        return set_error(KFX_E_NODEVICE, "kfx_sdf_summary_create: hipMalloc");
    }
    *out = s;
    return kfx_sdf_summary_invalidate(s, nullptr); // nothing is known about the volume's contents yet
}

extern "C" int kfx_sdf_summary_create(kfx_sdf_summary** out, const kfx_volume* vol) { return summary_create(out, vol, 8); }
extern "C" int kfx_sdf_summary_create_h(kfx_sdf_summary** out, const kfx_volume* vol) { return summary_create(out, vol, 4); }

extern "C" int kfx_sdf_summary_destroy(kfx_sdf_summary* s)
{
    if (!s) return 0;
    (void)hipDeviceSynchronize();   // a table build may still be about to publish its count
    if (s->R) (void)hipFree(s->R);
    if (s->C) (void)hipFree(s->C);
    if (s->d_count) (void)hipFree(s->d_count);
    if (s->h_skippable) (void)hipHostFree(s->h_skippable);
    else if (s->d_skippable) (void)hipFree(s->d_skippable);
    delete s;
    return 0;
}

extern "C" int kfx_sdf_summary_rebuild(kfx_sdf_summary* s, kfx_stream stream)
{
    if (!s) return set_error(KFX_E_NULL, "kfx_sdf_summary_rebuild: null summary");
    const long long n = (long long)s->nbx * s->nby * s->nbz;
    const int aligned16 = ((((uintptr_t)s->base) | s->pitch | s->img_pitch) & 15) == 0;
    if (s->cell_bytes == 4)
        hipLaunchKernelGGL(k_summary_rebuild<4>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, s->R, s->base, s->pitch, s->img_pitch,
                           s->w, s->h, s->d, s->nbx, s->nby, s->nbz, aligned16);
    else
        hipLaunchKernelGGL(k_summary_rebuild<8>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, s->R, s->base, s->pitch, s->img_pitch,
                           s->w, s->h, s->d, s->nbx, s->nby, s->nbz, aligned16);
    s->c_dirty = 2;
    return check_launch("kfx_sdf_summary_rebuild");
}

// After the volume was written by anything that does not track (memcpy, LoadPXM, SdfSphere, an untracked SdfFuse):
// every brick becomes "unknown", so the march samples everywhere until tracked updates re-establish ranges.
extern "C" int kfx_sdf_summary_invalidate(kfx_sdf_summary* s, kfx_stream stream)
{
    if (!s) return set_error(KFX_E_NULL, "kfx_sdf_summary_invalidate: null summary");
    const size_t n = (size_t)s->nbx * s->nby * s->nbz;
    hipLaunchKernelGGL(k_summary_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s->R, n, -__builtin_inff(), __builtin_inff(), 2);
    s->c_dirty = 2;
    return check_launch("kfx_sdf_summary_invalidate");
}

// SdfReset(vol, trunc_dist) of the WHOLE volume with the summary set to match: every cell = trunc_dist (NaN: never observed;
// half cells: trunc_dist rounded to half, the value the cells then hold)
static int reset_tracked(const kfx_volume* vol, kfx_sdf_summary* s, float trunc_dist, kfx_stream stream, int cell_bytes, const char* name)
{
    if (!s) return set_error(KFX_E_NULL, cell_bytes == 4 ? "kfx_sdf_reset_tracked_h: null summary" : "kfx_sdf_reset_tracked: null summary");
    if (s->cell_bytes != cell_bytes) return set_error(KFX_E_SHAPE, "SdfReset(tracked): the summary was created for the other cell type");
    int ox, oy, oz;
    if (int e = summary_view_offset(s, vol, &ox, &oy, &oz)) return e;
    if (ox || oy || oz || (int)vol->w != s->w || (int)vol->h != s->h || (int)vol->d != s->d)
        return set_error(KFX_E_SHAPE, "kfx_sdf_reset_tracked: resets the whole volume only (use kfx_sdf_reset + kfx_sdf_summary_invalidate for views)");
    if (int e = cell_bytes == 4 ? kfx_sdf_reset_h(vol, trunc_dist, stream) : kfx_sdf_reset(vol, trunc_dist, stream)) return e;
    const size_t n = (size_t)s->nbx * s->nby * s->nbz;
    const bool nan = trunc_dist != trunc_dist;
    const float v = cell_bytes == 4 ? __half2float(__float2half_rn(trunc_dist)) : trunc_dist;
    hipLaunchKernelGGL(k_summary_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, s->R, n,
                       nan ? __builtin_inff() : v, nan ? -__builtin_inff() : v, nan ? 1 : 0);
    s->c_dirty = 2;
    return check_launch(name);
}

extern "C" int kfx_sdf_reset_tracked(const kfx_volume* vol, kfx_sdf_summary* s, float trunc_dist, kfx_stream stream)
{
    return reset_tracked(vol, s, trunc_dist, stream, 8, "kfx_sdf_reset_tracked");
}

extern "C" int kfx_sdf_reset_tracked_h(const kfx_volume* vol, kfx_sdf_summary* s, float trunc_dist, kfx_stream stream)
{
    return reset_tracked(vol, s, trunc_dist, stream, 4, "kfx_sdf_reset_tracked_h");
}
