// bricks.hip -- sparse brick snapshots (include/kfx_bricks.h): which 8 x 8 x 8 bricks of a view differ from the fill cell, their ids
// in ascending order, their cells packed, and the way back.  The brick grid, the scratch and the refusals are bricks_host.h's.
//
//   k_brick_flags          the plan's one streaming read of the view, organised by volume rows: a workgroup owns a run of 1 KiB of
//                          cells along x (16 bricks of SDF_t, 32 of the 4-byte cells) in one (by, bz) -- 64 rows -- and each wave
//                          sweeps 16 of those rows, a lane one 16-byte segment of the address space (one load where the segment lies
//                          inside the run, cell by cell at a run's unaligned head and tail).  Words are compared with the fill's;
//                          a lane keeps what it found per brick in two registers (a segment meets two bricks at the most), ORs
//                          them into the workgroup's LDS flags once, and the workgroup writes one flag byte per brick it owns.
//   k_brick_count          live bricks per scan block of 256 bricks (ballot + popcount)
//   k_brick_scan_partials  one wave: exclusive offsets of the scan blocks, and the total
//   k_brick_ids            the ids of the live bricks at the scanned offsets
//   k_brick_move           pack / unpack: 16 bytes of the payload per lane (fully coalesced: a brick is 4 or 2 KiB, one or half a
//                          workgroup), the volume side 16 bytes where the row segment is aligned and inside the view, cell by cell
//                          otherwise; unpack writes cells inside the view only.
// No global atomics, nothing between workgroups of one launch: ordering comes from the stream.
// All but k_brick_move's own indexing live in bricks_device.h, which brick_pool.hip (include/kfx_brick_pool.h) shares.
#include "bricks_device.h"

using namespace kfx;

// Entry i of the list: brick ids[i] of the view <-> cells[i][8][8][8] (brick_move_lane)
template <int CELL, bool UNPACK>
__global__ __launch_bounds__(256) void k_brick_move(const BrickArgs a, const unsigned* __restrict__ ids, unsigned char* cells, const unsigned n)
{
    constexpr int TPB = BrickLanes<CELL>::TPB;
    const unsigned i = blockIdx.x * (256 / TPB) + threadIdx.x / TPB;
    if (i >= n) return;
    brick_move_lane<CELL, UNPACK>(a, ids[i], cells + (size_t)i * (BRICK_CELLS * CELL), (int)(threadIdx.x % TPB));
}

static int read_word(unsigned long long* host, const void* dev, hipStream_t st)
{
    hipError_t e = hipMemcpyAsync(host, dev, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : set_error((int)e, hipGetErrorString(e));
}

extern "C" size_t kfx_bricks_scratch_bytes(const kfx_volume* vol, int cell)
{
    BrickSetup s;
    if (brick_setup(s, vol, cell, 0.0f, "kfx_bricks_scratch_bytes")) return 0;
    return brick_scratch(s.g).bytes;
}

extern "C" int kfx_bricks_plan(const kfx_volume* vol, int cell, float fill, void* scratch, size_t scratch_bytes, unsigned long long* n_live, kfx_stream stream)
{
    const char* const what = "kfx_bricks_plan";
    BrickSetup s;
    if (int e = brick_setup(s, vol, cell, fill, what)) return e;
    if (!n_live) return fail_rule(what, KFX_E_NULL, "null n_live");
    if (int e = refuse(brick_check_scratch(s.g, scratch, scratch_bytes), what)) return e;
    const BrickScratch lay = brick_scratch(s.g);
    unsigned char* const base = (unsigned char*)scratch;
    unsigned char* const flags = base + lay.flags;
    const hipStream_t st = (hipStream_t)stream;
    for_cell_bytes(s.cb, [&](auto cb) {
        constexpr int CELL = decltype(cb)::value;
        const dim3 grid((unsigned)ceil_div(s.g.w, 1024 / CELL), (unsigned)s.g.nby, (unsigned)s.g.nbz);
        hipLaunchKernelGGL(k_brick_flags<CELL>, grid, dim3(256), 0, st, s.a, flags);
    });
    hipLaunchKernelGGL(k_brick_count, dim3((unsigned)s.g.nblk), dim3(256), 0, st, flags, s.a.nb, (unsigned*)(base + lay.part));
    hipLaunchKernelGGL(k_brick_scan_partials, dim3(1), dim3(64), 0, st, (const unsigned*)(base + lay.part), (unsigned)s.g.nblk, (unsigned*)(base + lay.base),
                       (unsigned long long*)(base + lay.hdr));
    if (int e = check_launch(what)) return e;
    return read_word(n_live, base + lay.hdr, st);
}

extern "C" int kfx_bricks_pack(const kfx_volume* vol, int cell, float fill, const void* scratch, size_t scratch_bytes, unsigned long long n_live,
                               unsigned* ids, void* cells, kfx_stream stream)
{
    const char* const what = "kfx_bricks_pack";
    BrickSetup s;
    if (int e = brick_setup(s, vol, cell, fill, what)) return e;
    if (int e = refuse(brick_check_scratch(s.g, scratch, scratch_bytes), what)) return e;
    if (n_live > s.g.nb) return fail_rule(what, KFX_E_RANGE, "n_live is not the plan's");
    if (int e = refuse(brick_check_lists(ids, cells, n_live), what)) return e;
    const BrickScratch lay = brick_scratch(s.g);
    const unsigned char* const base = (const unsigned char*)scratch;
    const hipStream_t st = (hipStream_t)stream;
    unsigned long long planned = 0;
    if (int e = read_word(&planned, base + lay.hdr, st)) return e;
    if (planned != n_live) return fail_rule(what, KFX_E_RANGE, "n_live is not the plan's");
    if (n_live == 0) return 0;
    const unsigned n = (unsigned)n_live;
    hipLaunchKernelGGL(k_brick_ids, dim3((unsigned)s.g.nblk), dim3(256), 0, st, base + lay.flags, s.a.nb, (const unsigned*)(base + lay.base), n, ids);
    for_cell_bytes(s.cb, [&](auto cb) {
        constexpr int CELL = decltype(cb)::value;
        constexpr unsigned PER_GROUP = 256 / (BRICK_CELLS * CELL / 16);   // bricks per workgroup
        hipLaunchKernelGGL((k_brick_move<CELL, false>), dim3((n + PER_GROUP - 1) / PER_GROUP), dim3(256), 0, st, s.a, (const unsigned*)ids,
                           (unsigned char*)cells, n);
    });
    return check_launch(what);
}

extern "C" int kfx_bricks_unpack(const kfx_volume* vol, int cell, const unsigned* ids, const void* cells, unsigned long long n_entries, kfx_stream stream)
{
    const char* const what = "kfx_bricks_unpack";
    BrickSetup s;
    if (int e = brick_setup(s, vol, cell, 0.0f, what)) return e;
    if (int e = refuse(brick_check_lists(ids, cells, n_entries), what)) return e;
    if (n_entries == 0) return 0;
    const unsigned n = (unsigned)n_entries;
    for_cell_bytes(s.cb, [&](auto cb) {
        constexpr int CELL = decltype(cb)::value;
        constexpr unsigned PER_GROUP = 256 / (BRICK_CELLS * CELL / 16);
        hipLaunchKernelGGL((k_brick_move<CELL, true>), dim3((n + PER_GROUP - 1) / PER_GROUP), dim3(256), 0, (hipStream_t)stream, s.a, ids,
                           (unsigned char*)const_cast<void*>(cells), n);
    });
    return check_launch(what);
}
