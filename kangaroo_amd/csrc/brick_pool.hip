// brick_pool.hip -- the brick pool (include/kfx_brick_pool.h): spilled 8 x 8 x 8 bricks under world keys in device memory of the
// caller, put in and taken out by stream-ordered launches.  The layout, the refusals and the rules of the pool -- which keys lie in a
// box, which slot a rank takes, how the header changes -- are brick_pool_host.h's; the classification of a view's bricks, the scan and
// the move of a brick are bricks_device.h's, shared with bricks.hip.
//
//   k_pool_init     every key free, free[i] = capacity - 1 - i, the header
//   k_pool_match    flags[slot] = 1 where the slot is occupied and its key lies in the box (one 16-byte load per slot)
//   k_pool_take     the flagged slots in ascending order (block_exclusive_scan at the scanned offsets): list[i] = the i-th of them,
//                   its key set free, free[free_n + i] = the slot
//   k_pool_put      the r-th live brick of the view -> slot free[free_n - 1 - r]: its key, and its cells (brick_move_lane)
//   k_pool_get      list[i], a slot just taken -> the brick of the view its key names (brick_move_lane, cells inside the view only)
//   k_pool_header   one workgroup: the header after a spill / a restore / a discard (brick_pool_after_spill, brick_pool_after_take)
//   k_pool_gather   cells_out[i] = the cells of slot slots[i], 16 bytes per lane
// No read-back: a grid covers every brick of the view (every slot of the pool) and a kernel reads how many of them count from the
// scratch's first word, which the scan before it wrote.  A kernel that reads free_n reads what the header kernel of the step before
// left there; nothing writes the header but k_pool_init and k_pool_header.  No global atomics, nothing between workgroups of one
// launch: ordering comes from the stream, so the pool's bytes are a function of the sequence of calls.
#include "bricks_device.h"
#include "brick_pool_host.h"

using namespace kfx;

// the parts of a pool, as the kernels take them
struct PoolArgs {
    BrickPoolHeader* hdr;
    BrickPoolKey* keys;
    unsigned* free;
    unsigned char* cells;
    unsigned capacity;
};

__global__ __launch_bounds__(256) void k_pool_init(const PoolArgs p, const unsigned cell)
{
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.capacity) {
        p.keys[i] = BrickPoolKey{0, 0, 0, BRICK_POOL_FREE};
        p.free[i] = p.capacity - 1 - i;
    }
    if (i == 0) *p.hdr = BrickPoolHeader{p.capacity, 0, 0, 0, cell, p.capacity};
}

__global__ __launch_bounds__(256) void k_pool_match(const PoolArgs p, const BrickPoolBox box, unsigned char* __restrict__ flags)
{
    const unsigned slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= p.capacity) return;
    const BrickPoolKey k = p.keys[slot];
    unsigned id;
    flags[slot] = k.state == BRICK_POOL_OCCUPIED && brick_pool_key_in_box(box, k.bx, k.by, k.bz, &id) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_pool_take(const PoolArgs p, const unsigned char* __restrict__ flags, const unsigned* __restrict__ base,
                                                   unsigned* __restrict__ list)
{
    __shared__ unsigned lds[4];
    const unsigned slot = blockIdx.x * BRICK_SCAN_BLOCK + threadIdx.x;
    const unsigned f = slot < p.capacity && flags[slot] != 0 ? 1u : 0u;
    unsigned total;
    const unsigned i = block_exclusive_scan<unsigned, 4>(f, lds, &total) + base[blockIdx.x];
    if (!f || i >= p.capacity) return;
    list[i] = slot;
    p.keys[slot].state = BRICK_POOL_FREE;
    const long long at = brick_pool_push_index(brick_pool_free_n(p.hdr->free_n, p.capacity), i, p.capacity);
    if (at >= 0) p.free[at] = slot;
}

// grid: the bricks of the view (at most capacity of them can find a slot), BrickLanes::PER_GROUP per workgroup
template <int CELL>
__global__ __launch_bounds__(256) void k_pool_put(const PoolArgs p, const BrickArgs a, const BrickPoolBox box, const unsigned long long* __restrict__ n_live,
                                                  const unsigned* __restrict__ ids)
{
    constexpr int TPB = BrickLanes<CELL>::TPB;
    const unsigned r = blockIdx.x * (256 / TPB) + threadIdx.x / TPB;
    if (r >= *n_live || r >= a.nb) return;
    const long long at = brick_pool_spill_index(brick_pool_free_n(p.hdr->free_n, p.capacity), r);
    if (at < 0) return;                                   // dropped
    const unsigned slot = p.free[at], id = ids[r];
    if (!brick_pool_slot_ok(slot, p.capacity) || id >= a.nb) return;
    const int t = (int)(threadIdx.x % TPB);
    if (t == 0) p.keys[slot] = brick_pool_key_of(box, id);
    brick_move_lane<CELL, false>(a, id, p.cells + (size_t)slot * (BRICK_CELLS * CELL), t);
}

// grid: min(bricks of the view, capacity) entries -- a pool holds a key once, so no more slots than the view has bricks were taken
template <int CELL>
__global__ __launch_bounds__(256) void k_pool_get(const PoolArgs p, const BrickArgs a, const BrickPoolBox box, const unsigned long long* __restrict__ n_taken,
                                                  const unsigned* __restrict__ list)
{
    constexpr int TPB = BrickLanes<CELL>::TPB;
    const unsigned i = blockIdx.x * (256 / TPB) + threadIdx.x / TPB;
    if (i >= *n_taken || i >= p.capacity) return;
    const unsigned slot = list[i];
    if (!brick_pool_slot_ok(slot, p.capacity)) return;
    const BrickPoolKey k = p.keys[slot];
    unsigned id;
    if (!brick_pool_key_in_box(box, k.bx, k.by, k.bz, &id)) return;
    brick_move_lane<CELL, true>(a, id, p.cells + (size_t)slot * (BRICK_CELLS * CELL), (int)(threadIdx.x % TPB));
}

enum { POOL_AFTER_SPILL = 0, POOL_AFTER_RESTORE = 1, POOL_AFTER_DISCARD = 2 };
__global__ __launch_bounds__(64) void k_pool_header(const PoolArgs p, const unsigned long long* __restrict__ count, const int what)
{
    if (threadIdx.x != 0) return;
    BrickPoolHeader h = *p.hdr;
    if (what == POOL_AFTER_SPILL) brick_pool_after_spill(h, *count, p.capacity);
    else brick_pool_after_take(h, *count, p.capacity, what == POOL_AFTER_RESTORE);
    *p.hdr = h;
}

// a lane: 16 bytes; a brick: TPB lanes
template <int CELL>
__global__ __launch_bounds__(256) void k_pool_gather(const PoolArgs p, const unsigned* __restrict__ slots, const unsigned n, unsigned char* __restrict__ out)
{
    constexpr int TPB = BrickLanes<CELL>::TPB;
    const unsigned i = blockIdx.x * (256 / TPB) + threadIdx.x / TPB;
    if (i >= n) return;
    const unsigned slot = slots[i];
    if (!brick_pool_slot_ok(slot, p.capacity)) return;
    const size_t t = threadIdx.x % TPB;
    const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p.cells + (size_t)slot * (BRICK_CELLS * CELL) + t * 16));
    __builtin_nontemporal_store(v, reinterpret_cast<v4u*>(out + (size_t)i * (BRICK_CELLS * CELL) + t * 16));
}

// ---- the host side ----
// what every entry point derives from (pool, pool_bytes, cell, capacity), after the checks
struct PoolSetup {
    size_t cb;
    BrickPoolLayout lay;
    PoolArgs p;
};
static int pool_setup(PoolSetup& s, const void* pool, size_t pool_bytes, int cell, unsigned long long capacity, const char* what)
{
    if (int e = refuse(brick_pool_check_kind(cell, capacity, s.cb), what)) return e;
    if (int e = refuse(brick_pool_check_pool(pool, pool_bytes, s.cb, capacity), what)) return e;
    s.lay = brick_pool_layout(s.cb, capacity);
    unsigned char* const base = (unsigned char*)const_cast<void*>(pool);
    s.p = PoolArgs{(BrickPoolHeader*)(base + s.lay.hdr), (BrickPoolKey*)(base + s.lay.keys), (unsigned*)(base + s.lay.free), base + s.lay.cells, (unsigned)capacity};
    return 0;
}

// the scratch of a call, carved
struct PoolScratch {
    unsigned long long* count;
    unsigned char* flags;
    unsigned *part, *base, *list;
};
static PoolScratch pool_scratch(void* scratch, const BrickPoolScratch& lay)
{
    unsigned char* const b = (unsigned char*)scratch;
    return PoolScratch{(unsigned long long*)(b + lay.hdr), b + lay.flags, (unsigned*)(b + lay.part), (unsigned*)(b + lay.base), (unsigned*)(b + lay.list)};
}

static BrickPoolBox pool_box(const int key0[3], int nbx, int nby, int nbz) { return BrickPoolBox{{key0[0], key0[1], key0[2]}, {nbx, nby, nbz}}; }

// The slots whose key lies in the box leave the pool: flags, scan, list + free stack; sc.count then holds how many.  The header is
// the caller's to update (k_pool_header), after whatever reads the list.
static void enqueue_take(const PoolSetup& s, const BrickPoolBox& box, const PoolScratch& sc, hipStream_t st)
{
    const unsigned nblk = (s.p.capacity + BRICK_SCAN_BLOCK - 1) / BRICK_SCAN_BLOCK;
    hipLaunchKernelGGL(k_pool_match, dim3(nblk), dim3(256), 0, st, s.p, box, sc.flags);
    launch_brick_scan(sc.flags, s.p.capacity, nblk, sc.part, sc.base, sc.count, st);
    hipLaunchKernelGGL(k_pool_take, dim3(nblk), dim3(256), 0, st, s.p, (const unsigned char*)sc.flags, (const unsigned*)sc.base, sc.list);
}
static void enqueue_header(const PoolSetup& s, const PoolScratch& sc, int what, hipStream_t st)
{
    hipLaunchKernelGGL(k_pool_header, dim3(1), dim3(64), 0, st, s.p, (const unsigned long long*)sc.count, what);
}

extern "C" size_t kfx_brick_pool_bytes(int cell, unsigned long long capacity)
{
    size_t cb;
    if (refuse(brick_pool_check_kind(cell, capacity, cb), "kfx_brick_pool_bytes")) return 0;
    return brick_pool_layout(cb, capacity).bytes;
}

extern "C" size_t kfx_brick_pool_scratch_bytes(const kfx_volume* view, int cell, unsigned long long capacity)
{
    const char* const what = "kfx_brick_pool_scratch_bytes";
    size_t cb;
    BrickSetup v;
    if (!view || !view->ptr) { fail_rule(what, KFX_E_NULL, "null view"); return 0; }
    if (refuse(brick_pool_check_kind(cell, capacity, cb), what)) return 0;
    if (brick_setup(v, view, cell, 0.0f, what)) return 0;
    return brick_pool_scratch(v.g.nb, capacity).bytes;
}

extern "C" int kfx_brick_pool_init(void* pool, size_t pool_bytes, int cell, unsigned long long capacity, kfx_stream stream)
{
    const char* const what = "kfx_brick_pool_init";
    PoolSetup s;
    if (!pool) return fail_rule(what, KFX_E_NULL, "null pool");
    if (int e = pool_setup(s, pool, pool_bytes, cell, capacity, what)) return e;
    hipLaunchKernelGGL(k_pool_init, dim3((s.p.capacity + 255) / 256), dim3(256), 0, (hipStream_t)stream, s.p, (unsigned)cell);
    return check_launch(what);
}

// the checks spill and restore share, in the header's order
static int view_call_setup(PoolSetup& s, BrickSetup& v, BrickPoolBox& box, PoolScratch& sc, void* pool, size_t pool_bytes, int cell, unsigned long long capacity,
                           const kfx_volume* view, float fill, const int key0[3], void* scratch, size_t scratch_bytes, const char* what)
{
    if (!pool) return fail_rule(what, KFX_E_NULL, "null pool");
    if (!view || !view->ptr) return fail_rule(what, KFX_E_NULL, "null view");
    if (!key0) return fail_rule(what, KFX_E_NULL, "null key0");
    if (!scratch) return fail_rule(what, KFX_E_NULL, "null scratch");
    if (int e = pool_setup(s, pool, pool_bytes, cell, capacity, what)) return e;
    if (int e = brick_setup(v, view, cell, fill, what)) return e;
    if (int e = refuse(brick_pool_check_scratch(v.g.nb, capacity, scratch, scratch_bytes), what)) return e;
    box = pool_box(key0, v.g.nbx, v.g.nby, v.g.nbz);
    if (int e = refuse(brick_pool_check_keys(box.key0, box.nb), what)) return e;
    sc = pool_scratch(scratch, brick_pool_scratch(v.g.nb, capacity));
    return 0;
}

extern "C" int kfx_brick_pool_spill(void* pool, size_t pool_bytes, int cell, unsigned long long capacity, const kfx_volume* view, float fill, const int key0[3],
                                    void* scratch, size_t scratch_bytes, kfx_stream stream)
{
    const char* const what = "kfx_brick_pool_spill";
    PoolSetup s;
    BrickSetup v;
    BrickPoolBox box;
    PoolScratch sc;
    if (int e = view_call_setup(s, v, box, sc, pool, pool_bytes, cell, capacity, view, fill, key0, scratch, scratch_bytes, what)) return e;
    const hipStream_t st = (hipStream_t)stream;
    // what the pool holds of these keys goes first: a key is in the pool once
    enqueue_take(s, box, sc, st);
    enqueue_header(s, sc, POOL_AFTER_DISCARD, st);
    // the live bricks of the view, in ascending id, into the slots on top of the stack
    const unsigned nb = v.a.nb, nblk = (unsigned)v.g.nblk;
    launch_brick_flags(v, sc.flags, st);
    launch_brick_scan(sc.flags, nb, nblk, sc.part, sc.base, sc.count, st);
    hipLaunchKernelGGL(k_brick_ids, dim3(nblk), dim3(256), 0, st, (const unsigned char*)sc.flags, nb, (const unsigned*)sc.base, nb, sc.list);
    const unsigned entries = nb < s.p.capacity ? nb : s.p.capacity;
    for_cell_bytes(s.cb, [&](auto cb) {
        constexpr int CELL = decltype(cb)::value;
        constexpr unsigned PER_GROUP = BrickLanes<CELL>::PER_GROUP;
        hipLaunchKernelGGL(k_pool_put<CELL>, dim3((entries + PER_GROUP - 1) / PER_GROUP), dim3(256), 0, st, s.p, v.a, box, (const unsigned long long*)sc.count,
                           (const unsigned*)sc.list);
    });
    enqueue_header(s, sc, POOL_AFTER_SPILL, st);
    return check_launch(what);
}

extern "C" int kfx_brick_pool_restore(void* pool, size_t pool_bytes, int cell, unsigned long long capacity, const kfx_volume* view, const int key0[3],
                                      void* scratch, size_t scratch_bytes, kfx_stream stream)
{
    const char* const what = "kfx_brick_pool_restore";
    PoolSetup s;
    BrickSetup v;
    BrickPoolBox box;
    PoolScratch sc;
    if (int e = view_call_setup(s, v, box, sc, pool, pool_bytes, cell, capacity, view, 0.0f, key0, scratch, scratch_bytes, what)) return e;
    const hipStream_t st = (hipStream_t)stream;
    enqueue_take(s, box, sc, st);
    const unsigned entries = v.a.nb < s.p.capacity ? v.a.nb : s.p.capacity;
    for_cell_bytes(s.cb, [&](auto cb) {
        constexpr int CELL = decltype(cb)::value;
        constexpr unsigned PER_GROUP = BrickLanes<CELL>::PER_GROUP;
        hipLaunchKernelGGL(k_pool_get<CELL>, dim3((entries + PER_GROUP - 1) / PER_GROUP), dim3(256), 0, st, s.p, v.a, box, (const unsigned long long*)sc.count,
                           (const unsigned*)sc.list);
    });
    enqueue_header(s, sc, POOL_AFTER_RESTORE, st);
    return check_launch(what);
}

extern "C" int kfx_brick_pool_discard(void* pool, size_t pool_bytes, int cell, unsigned long long capacity, const int nb[3], const int key0[3], void* scratch,
                                      size_t scratch_bytes, kfx_stream stream)
{
    const char* const what = "kfx_brick_pool_discard";
    PoolSetup s;
    if (!pool) return fail_rule(what, KFX_E_NULL, "null pool");
    if (!nb) return fail_rule(what, KFX_E_NULL, "null nb");
    if (!key0) return fail_rule(what, KFX_E_NULL, "null key0");
    if (!scratch) return fail_rule(what, KFX_E_NULL, "null scratch");
    if (int e = pool_setup(s, pool, pool_bytes, cell, capacity, what)) return e;
    if (nb[0] < 1 || nb[1] < 1 || nb[2] < 1) return fail_rule(what, KFX_E_SHAPE, "a key box has at least one key per axis");
    if ((unsigned long long)nb[0] * (unsigned long long)nb[1] > BRICK_MAX || (unsigned long long)nb[0] * (unsigned long long)nb[1] * (unsigned long long)nb[2] > BRICK_MAX)
        return fail_rule(what, KFX_E_RANGE, "more than 2^31 - 1 keys");
    if (int e = refuse(brick_pool_check_scratch(0, capacity, scratch, scratch_bytes), what)) return e;
    const BrickPoolBox box = pool_box(key0, nb[0], nb[1], nb[2]);
    if (int e = refuse(brick_pool_check_keys(box.key0, box.nb), what)) return e;
    const PoolScratch sc = pool_scratch(scratch, brick_pool_scratch(0, capacity));
    enqueue_take(s, box, sc, (hipStream_t)stream);
    enqueue_header(s, sc, POOL_AFTER_DISCARD, (hipStream_t)stream);
    return check_launch(what);
}

extern "C" int kfx_brick_pool_stats(const void* pool, size_t pool_bytes, int cell, unsigned long long capacity, unsigned long long out[4], kfx_stream stream)
{
    const char* const what = "kfx_brick_pool_stats";
    PoolSetup s;
    if (!pool) return fail_rule(what, KFX_E_NULL, "null pool");
    if (!out) return fail_rule(what, KFX_E_NULL, "null out");
    if (int e = pool_setup(s, pool, pool_bytes, cell, capacity, what)) return e;
    unsigned long long h[4];
    hipError_t e = hipMemcpyAsync(h, s.p.hdr, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return set_error((int)e, hipGetErrorString(e));
    out[0] = capacity - brick_pool_free_n(h[0], capacity);
    out[1] = h[1]; out[2] = h[2]; out[3] = h[3];
    return 0;
}

extern "C" int kfx_brick_pool_gather(const void* pool, size_t pool_bytes, int cell, unsigned long long capacity, const unsigned* slots, unsigned long long n,
                                     void* cells_out, kfx_stream stream)
{
    const char* const what = "kfx_brick_pool_gather";
    PoolSetup s;
    if (!pool) return fail_rule(what, KFX_E_NULL, "null pool");
    if (int e = pool_setup(s, pool, pool_bytes, cell, capacity, what)) return e;
    if (int e = refuse(brick_check_lists(slots, cells_out, n), what)) return e;
    if (n == 0) return 0;
    for_cell_bytes(s.cb, [&](auto cb) {
        constexpr int CELL = decltype(cb)::value;
        constexpr unsigned PER_GROUP = BrickLanes<CELL>::PER_GROUP;
        hipLaunchKernelGGL(k_pool_gather<CELL>, dim3(((unsigned)n + PER_GROUP - 1) / PER_GROUP), dim3(256), 0, (hipStream_t)stream, s.p, slots, (unsigned)n,
                           (unsigned char*)cells_out);
    });
    return check_launch(what);
}
