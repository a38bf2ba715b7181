// slab_comm.hip -- the in-process transports behind kfx_comm (include/kfx_slab.h).  threads (kfx_comm_create_threads): ranks = host
// threads sharing the device, every collective a barrier of all ranks -- ONE skeleton, collective(), holds that protocol, and all_reduce,
// exchange_v, broadcast and all_to_all / all_gather supply a pre-check, the slots they publish and a body between the barriers.
// threads, p2p (kfx_comm_create_threads_p2p): the neighbour exchanges matched pairwise with a deadline, as RCCL matches send / recv.
// loop-back (kfx_comm_create_loopback): one rank of a `world`-rank job by itself.  RCCL: comm_rccl.cpp; what uses a transport: slab.hip.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <new>

#include "kfx_device.h"
#include "host_args.h"
#include "../../include/kfx_slab.h"

namespace kfx {

// ---- threads transport: reduction over the ranks' buffers by one kernel -------------------------------------------
constexpr int MAX_THREAD_RANKS = 16;
struct PtrList { void* p[MAX_THREAD_RANKS]; };

template <typename T, int OP>
__global__ __launch_bounds__(256) void k_group_reduce(PtrList bufs, int world, size_t count)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    T acc = reinterpret_cast<const T*>(bufs.p[0])[i];
    for (int r = 1; r < world; ++r) {
        const T v = reinterpret_cast<const T*>(bufs.p[r])[i];
        if constexpr (OP == 0) acc = v < acc ? v : acc;
        else acc = acc + v;   // rank order: every rank ends up with the same bits
    }
    for (int r = 0; r < world; ++r) reinterpret_cast<T*>(bufs.p[r])[i] = acc;
}

struct ThreadGroup {
    int world = 0;
    std::mutex m;
    std::condition_variable cv;
    int arrived = 0;
    unsigned long generation = 0;
    // what a rank shows its peers in a collective: what it SENDS down / up (all_to_all / all_gather: lo), or its buffer (all_reduce, broadcast)
    struct Slots { const void* send_lo; size_t bytes_lo; const void* send_hi; size_t bytes_hi; void* buf; };
    Slots slot[MAX_THREAD_RANKS];
    // per-rank error of a collective, double-buffered by the collective's sequence parity: a rank that has left collective k
    // and already entered k + 1 posts into the other set while a slower peer may still be reading k's in group_status(); the
    // set of k is written again in k + 2, which every rank enters only after it returned from k + 1 -- whose barriers all
    // ranks passed after they had returned from k (round-3 advice).  seq[r] is rank r's own count of collectives.
    std::atomic<int> err[2][MAX_THREAD_RANKS];
    unsigned seq[MAX_THREAD_RANKS] = {};
    // Point-to-point mode (kfx_comm_create_threads_p2p): the neighbour exchanges are matched PAIRWISE, in order, per directed link --
    // the way RCCL matches ncclSend / ncclRecv -- instead of being a barrier of all ranks: a rank with nothing to pass on does not
    // take part, ranks drift apart by whole frames (what kfx_slab_frame's pipelined frames are for), and a leg whose two sides
    // disagree -- one side skips it, or names another size -- does not fail at once: it BLOCKS, as it would on RCCL, until
    // `timeout_ms` have passed, and then reports KFX_E_TIMEOUT.  link[0][r]: r -> r + 1, link[1][r]: r -> r - 1; one message in
    // flight per link (the sender returns from its call once the receiver has taken the message).
    struct Link { const void* src = nullptr; size_t bytes = 0; bool full = false; };
    bool p2p = false;
    int timeout_ms = 0;
    Link link[2][MAX_THREAD_RANKS];
    ThreadGroup* dup_out = nullptr;   // threads_dup: the new group travels from rank 0 to the others through the old one
    ThreadGroup() { for (auto& set : err) for (auto& e : set) e.store(0); }

    void wait_all()
    {
        std::unique_lock<std::mutex> lk(m);
        const unsigned long g = generation;
        if (++arrived == world) {
            arrived = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return generation != g; });
        }
    }
};

static ThreadGroup* group_of(kfx_comm* c) { return static_cast<ThreadGroup*>(c->impl); }

// the first error any rank posted for the collective of parity `par`
static int group_status(const ThreadGroup* g, int par)
{
    for (int r = 0; r < g->world; ++r)
        if (const int e = g->err[par][r].load()) return e;
    return 0;
}

// ---- barrier mode: the one skeleton of a collective -------------------------------------------------------------------------
// Every rank passes both barriers whatever happened locally (a rank that returned early on its own error would leave its peers waiting
// on the condition variable for ever), the sequence number advances exactly once, and after the last barrier every rank returns the
// first error any rank posted for THIS collective: no return and no branch goes around a barrier or the increment.
//   pre: the caller's argument check (0: fine).  mine: this rank's slots, which the peers read after the first barrier.  takes_part:
//   whether this rank has a body to run.  body(g, par): between the barriers, on a rank without an error of its own; reads the peers'
//   slots (those of a peer whose err[par] is set mean nothing), enqueues on the stream, returns a status.  The stream is synchronised
//   after it: nobody reuses a buffer before its readers are done.
template <typename BODY>
static int collective(kfx_comm* c, kfx_stream stream, const char* who, int pre, const ThreadGroup::Slots& mine, bool takes_part, const BODY& body)
{
    ThreadGroup* g = group_of(c);
    const int r = c->rank;
    FirstError st;
    st(pre);
    if (!st.status) st(hip_status(hipStreamSynchronize((hipStream_t)stream), who));   // this rank's producers are done
    const int par = (int)(g->seq[r]++ & 1u);
    g->err[par][r].store(st.status);
    g->slot[r] = mine;
    g->wait_all();
    if (takes_part && !st.status) {
        st(body(g, par));
        if (!st.status) st(hip_status(hipStreamSynchronize((hipStream_t)stream), who));
        if (st.status) g->err[par][r].store(st.status);   // (atomic: a peer may be reading the slot: it sees 0 or an error; the final value counts)
    }
    g->wait_all();
    return group_status(g, par);
}

static int threads_all_reduce(kfx_comm* c, void* buf, size_t count, int op, kfx_stream stream)
{
    const char* who = "kfx_comm(threads) all_reduce";
    const int pre = (!buf && count) ? set_error(KFX_E_NULL, "kfx_comm(threads) all_reduce: null buffer") : 0;
    // rank 0 reduces for everybody, into every rank's buffer
    return collective(c, stream, who, pre, {nullptr, 0, nullptr, 0, buf}, c->rank == 0 && count, [&](ThreadGroup* g, int par) {
        if (group_status(g, par)) return 0;
        PtrList pl;
        for (int r = 0; r < g->world; ++r) pl.p[r] = g->slot[r].buf;
        const dim3 grid((unsigned)((count + 255) / 256));
        hipStream_t s = (hipStream_t)stream;
        if (op == KFX_COMM_MIN_I64) hipLaunchKernelGGL((k_group_reduce<long long, 0>), grid, dim3(256), 0, s, pl, g->world, count);
        else if (op == KFX_COMM_SUM_F32) hipLaunchKernelGGL((k_group_reduce<float, 1>), grid, dim3(256), 0, s, pl, g->world, count);
        else if (op == KFX_COMM_SUM_I32) hipLaunchKernelGGL((k_group_reduce<int, 1>), grid, dim3(256), 0, s, pl, g->world, count);
        else return set_error(KFX_E_RANGE, "kfx_comm all_reduce: unknown op");
        return check_launch(who);
    });
}

// One receive leg of an exchange: what neighbour `from` sends this way -- `sent` bytes at `src`, its slots -- into `recv`, which
// expects `bytes`; `unexpected` is the message for a neighbour that sends what this rank does not receive.
static int receive_leg(ThreadGroup* g, int par, int from, const void* src, size_t sent, void* recv, size_t bytes, const char* unexpected, hipStream_t s)
{
    if (g->err[par][from].load() != 0) return 0;
    if (!bytes) return sent ? set_error(KFX_E_SHAPE, unexpected) : 0;
    if (sent != bytes) return set_error(KFX_E_SHAPE, "kfx_comm exchange: neighbours disagree on the byte count");
    return hip_status(hipMemcpyAsync(recv, src, bytes, hipMemcpyDeviceToDevice, s), "kfx_comm(threads) exchange");
}

static int threads_exchange_v(kfx_comm* c, const void* send_lo, size_t bytes_send_lo, void* recv_lo, size_t bytes_recv_lo, const void* send_hi,
                              size_t bytes_send_hi, void* recv_hi, size_t bytes_recv_hi, kfx_stream stream)
{
    const int r = c->rank;
    const ThreadGroup::Slots mine{send_lo, r > 0 ? bytes_send_lo : 0, send_hi, r + 1 < c->world ? bytes_send_hi : 0, nullptr};
    return collective(c, stream, "kfx_comm(threads) exchange", 0, mine, true, [&](ThreadGroup* g, int par) {
        hipStream_t s = (hipStream_t)stream;
        FirstError st;
        if (r > 0)   // what rank - 1 sends upwards
            st(receive_leg(g, par, r - 1, g->slot[r - 1].send_hi, g->slot[r - 1].bytes_hi, recv_lo, bytes_recv_lo, "kfx_comm exchange: the lower neighbour sends what this rank does not receive", s));
        if (!st.status && r + 1 < g->world)   // what rank + 1 sends downwards
            st(receive_leg(g, par, r + 1, g->slot[r + 1].send_lo, g->slot[r + 1].bytes_lo, recv_hi, bytes_recv_hi, "kfx_comm exchange: the upper neighbour sends what this rank does not receive", s));
        return st.status;
    });
}

// Point-to-point mode: post the sends, take what the neighbours posted, wait until the own messages have been taken.  No barrier,
// no other rank involved; a leg without a partner -- or whose partner names another size -- blocks until the timeout.
static int threads_exchange_v_p2p(kfx_comm* c, const void* send_lo, size_t bytes_send_lo, void* recv_lo, size_t bytes_recv_lo, const void* send_hi,
                                  size_t bytes_send_hi, void* recv_hi, size_t bytes_recv_hi, kfx_stream stream)
{
    ThreadGroup* g = group_of(c);
    const int r = c->rank;
    const bool has_lo = r > 0, has_hi = r + 1 < g->world;
    const bool sl = has_lo && bytes_send_lo, rl = has_lo && bytes_recv_lo, sh = has_hi && bytes_send_hi, rh = has_hi && bytes_recv_hi;
    if (!sl && !rl && !sh && !rh) return 0;   // (as the RCCL transport: nothing to do, nobody to meet)
    if ((sl && !send_lo) || (rl && !recv_lo) || (sh && !send_hi) || (rh && !recv_hi)) return set_error(KFX_E_NULL, "kfx_comm(threads, p2p) exchange: null buffer");
    hipStream_t s = (hipStream_t)stream;
    FirstError st;
    st(hip_status(hipStreamSynchronize(s), "kfx_comm(threads, p2p) exchange"));   // this rank's producers are done
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(g->timeout_ms > 0 ? g->timeout_ms : 10000);
    std::unique_lock<std::mutex> lk(g->m);
    ThreadGroup::Link* up = &g->link[0][r];      // r -> r + 1
    ThreadGroup::Link* down = &g->link[1][r];    // r -> r - 1
    const auto post = [&](ThreadGroup::Link* l, const void* src, size_t bytes) {
        if (!g->cv.wait_until(lk, deadline, [&] { return !l->full; })) return false;   // (the previous message of this link was never taken)
        l->src = src; l->bytes = bytes; l->full = true;
        return true;
    };
    bool timed_out = false;
    if (!st.status && sh) timed_out = !post(up, send_hi, bytes_send_hi) || timed_out;
    if (!st.status && sl) timed_out = !post(down, send_lo, bytes_send_lo) || timed_out;
    g->cv.notify_all();
    // a message is taken only by a receive of ITS size: any other pairing waits (for ever on RCCL; here until the deadline)
    const auto take = [&](ThreadGroup::Link* l, void* dst, size_t bytes) {
        if (!g->cv.wait_until(lk, deadline, [&] { return l->full && l->bytes == bytes; })) return false;
        const void* src = l->src;
        lk.unlock();
        int e = hip_status(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s), "kfx_comm(threads, p2p) exchange");
        if (!e) e = hip_status(hipStreamSynchronize(s), "kfx_comm(threads, p2p) exchange");
        lk.lock();
        st(e);
        l->full = false;   // the sender may go on (its buffer has been read)
        g->cv.notify_all();
        return true;
    };
    if (!st.status && !timed_out && rl) timed_out = !take(&g->link[0][r - 1], recv_lo, bytes_recv_lo) || timed_out;   // what rank - 1 sends upwards
    if (!st.status && !timed_out && rh) timed_out = !take(&g->link[1][r + 1], recv_hi, bytes_recv_hi) || timed_out;   // what rank + 1 sends downwards
    // nobody reuses a send buffer before its reader is done
    if (!st.status && !timed_out && sh) timed_out = !g->cv.wait_until(lk, deadline, [&] { return !up->full || up->src != send_hi; }) || timed_out;
    if (!st.status && !timed_out && sl) timed_out = !g->cv.wait_until(lk, deadline, [&] { return !down->full || down->src != send_lo; }) || timed_out;
    if (timed_out) {
        // withdraw what was posted and never taken, so that a later exchange of this link starts clean
        if (sh && up->full && up->src == send_hi) up->full = false;
        if (sl && down->full && down->src == send_lo) down->full = false;
        g->cv.notify_all();
        return set_error(KFX_E_TIMEOUT, "kfx_comm(threads, p2p) exchange: a leg found no partner of its size in time (on RCCL this rank would hang: the two sides of a leg must derive the same byte count)");
    }
    return st.status;
}

static int threads_exchange_v_any(kfx_comm* c, const void* send_lo, size_t bsl, void* recv_lo, size_t brl, const void* send_hi, size_t bsh, void* recv_hi,
                                  size_t brh, kfx_stream stream)
{
    if (group_of(c)->p2p) return threads_exchange_v_p2p(c, send_lo, bsl, recv_lo, brl, send_hi, bsh, recv_hi, brh, stream);
    return threads_exchange_v(c, send_lo, bsl, recv_lo, brl, send_hi, bsh, recv_hi, brh, stream);
}

// kfx_comm::exchange of a transport = its exchange_v with what a rank sends a neighbour as large as what it receives from it
template <int (*EXCHANGE_V)(kfx_comm*, const void*, size_t, void*, size_t, const void*, size_t, void*, size_t, kfx_stream)>
static int exchange_equal(kfx_comm* c, const void* send_lo, void* recv_lo, size_t bytes_lo, const void* send_hi, void* recv_hi, size_t bytes_hi, kfx_stream stream)
{
    return EXCHANGE_V(c, send_lo, bytes_lo, recv_lo, bytes_lo, send_hi, bytes_hi, recv_hi, bytes_hi, stream);
}

static int threads_broadcast(kfx_comm* c, void* buf, size_t bytes, int root, kfx_stream stream)
{
    FirstError pre;
    if (root < 0 || root >= c->world) pre(set_error(KFX_E_RANGE, "kfx_comm broadcast: root"));
    if (!pre.status && !buf && bytes) pre(set_error(KFX_E_NULL, "kfx_comm(threads) broadcast: null buffer"));
    // the readers copy; the root keeps its buffer untouched until every reader is done
    return collective(c, stream, "kfx_comm(threads) broadcast", pre.status, {nullptr, 0, nullptr, 0, buf}, c->rank != root && bytes, [&](ThreadGroup* g, int par) {
        if (g->err[par][root].load() != 0) return 0;
        return hip_status(hipMemcpyAsync(buf, g->slot[root].buf, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), "kfx_comm(threads) broadcast");
    });
}

// all_to_all (gather = false): recv chunk r <- chunk `rank` of rank r's send; all_gather (gather = true): recv chunk r <- rank r's send
static int threads_mesh(kfx_comm* c, const void* send, void* recv, size_t bytes, bool gather, kfx_stream stream)
{
    const char* who = "kfx_comm(threads) all_to_all / all_gather";
    const int r = c->rank;
    const int pre = ((!send || !recv) && bytes) ? set_error(KFX_E_NULL, "kfx_comm(threads) all_to_all / all_gather: null buffer") : 0;
    return collective(c, stream, who, pre, {send, bytes, nullptr, 0, nullptr}, true, [&](ThreadGroup* g, int par) {
        for (int k = 0; k < g->world && bytes; ++k) {
            const int from = (r + k) % g->world;
            if (g->err[par][from].load() != 0) continue;
            if (g->slot[from].bytes_lo != bytes) return set_error(KFX_E_SHAPE, "kfx_comm all_to_all / all_gather: ranks disagree on the byte count");
            const unsigned char* src = static_cast<const unsigned char*>(g->slot[from].send_lo) + (gather ? 0 : (size_t)r * bytes);
            if (int e = hip_status(hipMemcpyAsync(static_cast<unsigned char*>(recv) + (size_t)from * bytes, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), who)) return e;
        }
        return 0;
    });
}

static int threads_all_to_all(kfx_comm* c, const void* send, void* recv, size_t bytes, kfx_stream stream) { return threads_mesh(c, send, recv, bytes, false, stream); }
static int threads_all_gather(kfx_comm* c, const void* send, void* recv, size_t bytes, kfx_stream stream) { return threads_mesh(c, send, recv, bytes, true, stream); }

static int threads_barrier(kfx_comm* c) { group_of(c)->wait_all(); return 0; }

static void threads_destroy(kfx_comm* c)
{
    if (c && c->impl && c->rank == 0) delete group_of(c);
    if (c) c->impl = nullptr;
}

static int threads_dup(kfx_comm* c, kfx_comm* out);

static void threads_fill(kfx_comm* c, ThreadGroup* g, int rank)
{
    c->rank = rank;
    c->world = g->world;
    c->impl = g;
    c->all_reduce = threads_all_reduce;
    c->exchange = exchange_equal<threads_exchange_v_any>;
    c->barrier = threads_barrier;
    c->destroy = threads_destroy;
    c->broadcast = threads_broadcast;
    c->all_to_all = threads_all_to_all;
    c->all_gather = threads_all_gather;
    c->exchange_v = threads_exchange_v_any;
    c->flags = KFX_COMM_HOST_BLOCKING;   // a collective returns when every rank has entered it
    c->dup = threads_dup;
}

// A second group over the same threads (every rank calls; rank 0 destroys the copy like the original: through its own table).  Two
// barriers of its own: it posts no error -- a failed allocation is every rank's null pointer.
static int threads_dup(kfx_comm* c, kfx_comm* out)
{
    if (!c || !out || !c->impl) return set_error(KFX_E_NULL, "kfx_comm(threads) dup: null argument");
    ThreadGroup* g = group_of(c);
    if (c->rank == 0) {
        ThreadGroup* n = new (std::nothrow) ThreadGroup;
        if (n) { n->world = g->world; n->p2p = g->p2p; n->timeout_ms = g->timeout_ms; }
        g->dup_out = n;
    }
    g->wait_all();
    ThreadGroup* n = g->dup_out;
    g->wait_all();   // (everybody has read it before a later dup overwrites it)
    if (!n) return set_error(KFX_E_RANGE, "kfx_comm(threads) dup: out of memory");
    threads_fill(out, n, c->rank);
    return 0;
}

} // namespace kfx

using namespace kfx;

static int create_threads(kfx_comm* comms, int world, bool p2p, int timeout_ms)
{
    if (!comms) return set_error(KFX_E_NULL, "kfx_comm_create_threads: null comms");
    if (world < 1 || world > MAX_THREAD_RANKS) return set_error(KFX_E_RANGE, "kfx_comm_create_threads: world in [1, 16]");
    ThreadGroup* g = new (std::nothrow) ThreadGroup;
    if (!g) return set_error(KFX_E_RANGE, "kfx_comm_create_threads: out of memory");
    g->world = world;
    g->p2p = p2p;
    g->timeout_ms = timeout_ms;
    for (int r = 0; r < world; ++r) threads_fill(&comms[r], g, r);
    return 0;
}

extern "C" int kfx_comm_create_threads(kfx_comm* comms, int world) { return create_threads(comms, world, false, 0); }
extern "C" int kfx_comm_create_threads_p2p(kfx_comm* comms, int world, int timeout_ms) { return create_threads(comms, world, true, timeout_ms); }

// ---- loop-back transport (kfx_slab.h): one rank of a `world`-rank job measured by itself ------------------------------
namespace {
int loop_copy(void* dst, const void* src, size_t bytes, kfx_stream stream)
{
    if (!bytes || !dst || !src || dst == src) return 0;
    return hip_status(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), "kfx_comm(loopback)");
}
int loop_all_reduce(kfx_comm*, void*, size_t, int, kfx_stream) { return 0; }   // nothing arrives: the buffer is the "sum"
// what would arrive over one leg: this rank's own opposite send buffer (the neighbour's is as large) -- the other one if that is null --,
// clipped to the receive size
int loop_leg(void* recv, size_t recv_bytes, const void* opposite, size_t opposite_bytes, const void* other, size_t other_bytes, kfx_stream stream)
{
    const size_t have = opposite ? opposite_bytes : other_bytes;
    return loop_copy(recv, opposite ? opposite : other, recv_bytes < have ? recv_bytes : have, stream);
}
int loop_exchange_v(kfx_comm* c, const void* send_lo, size_t bsl, void* recv_lo, size_t brl, const void* send_hi, size_t bsh, void* recv_hi,
                    size_t brh, kfx_stream stream)
{
    if (c->rank > 0) if (int e = loop_leg(recv_lo, brl, send_hi, bsh, send_lo, bsl, stream)) return e;
    if (c->rank + 1 < c->world) if (int e = loop_leg(recv_hi, brh, send_lo, bsl, send_hi, bsh, stream)) return e;
    return 0;
}
int loop_barrier(kfx_comm*) { return hip_status(hipDeviceSynchronize(), "kfx_comm(loopback) barrier"); }
void loop_destroy(kfx_comm* c) { if (c) c->impl = nullptr; }
int loop_broadcast(kfx_comm*, void*, size_t, int, kfx_stream) { return 0; }
int loop_all_to_all(kfx_comm* c, const void* send, void* recv, size_t bytes, kfx_stream stream) { return loop_copy(recv, send, bytes * (size_t)c->world, stream); }
int loop_all_gather(kfx_comm* c, const void* send, void* recv, size_t bytes, kfx_stream stream)
{
    for (int r = 0; r < c->world; ++r)
        if (int e = loop_copy(static_cast<unsigned char*>(recv) + (size_t)r * bytes, send, bytes, stream)) return e;
    return 0;
}
} // namespace

extern "C" int kfx_comm_create_loopback(kfx_comm* comm, int rank, int world)
{
    if (!comm) return set_error(KFX_E_NULL, "kfx_comm_create_loopback: null comm");
    if (world < 1 || rank < 0 || rank >= world) return set_error(KFX_E_RANGE, "kfx_comm_create_loopback: 0 <= rank < world");
    comm->rank = rank; comm->world = world; comm->impl = nullptr;
    comm->all_reduce = loop_all_reduce; comm->exchange = exchange_equal<loop_exchange_v>; comm->barrier = loop_barrier; comm->destroy = loop_destroy;
    comm->broadcast = loop_broadcast; comm->all_to_all = loop_all_to_all; comm->all_gather = loop_all_gather; comm->exchange_v = loop_exchange_v;
    comm->flags = 0;
    comm->dup = [](kfx_comm* c, kfx_comm* out) -> int { return kfx_comm_create_loopback(out, c->rank, c->world); };
    return 0;
}
