// slab.hip -- Z-slab partition of the TSDF volume across ranks (include/kfx_slab.h): the slab layout, the ghost-plane exchange, the
// input broadcast, the drivers of the nearest-hit composite (its kernels: composite.hip), and the exact march in its three
// generations -- the all-reduce cross-check, the hand-over, the hand-over pipelined over image row-tiles -- with their kernels.
// The collectives themselves belong to the transport behind kfx_comm (in-process: slab_comm.hip, RCCL: comm_rccl.cpp); this file
// only orders kernels and collectives on the caller's stream.  A step that fails locally does not keep the rank out of the
// collectives after it: FirstError (host_args.h).
// No reference counterpart (the reference is single-GPU); the host-side protocol is the one of
// kangaroo_amd/pipeline.py::SlabPipeline, so that C / C++ applications can use slabs without Python.
#include <atomic>
#include <cmath>

#include "kfx_device.h"
#include "host_args.h"
#include "raycast_ray.h"
#include "../../include/kfx_slab.h"
#include "slab_internal.h"

namespace kfx {

// ---- exact march: merging the per-rank states between rounds -------------------------------------------------------
// state planes (kfx.h, KFX_RAY_STATE_PLANES): 0 lambda, 1 last_sdf, 2 delta, 3 status, 4 touched, 5-7 normal, 8 shade.
// In a round exactly one rank touches a pixel, so SUM over ranks of (touched ? bits : 0) is that rank's state.
__global__ __launch_bounds__(256) void k_state_contrib(const int* __restrict__ state, int* __restrict__ contrib, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool touched = state[4 * n + i] != 0;
#pragma unroll
    for (int p = 0; p < 5; ++p) contrib[p * n + i] = touched ? state[p * n + i] : 0;
}

// after the all-reduce: adopt the touching rank's state; *flag |= 1 while any ray is still marching (status 0) or a hit
// awaits its normal (status 3)
__global__ __launch_bounds__(256) void k_state_merge(int* __restrict__ state, const int* __restrict__ contrib, size_t n, int merge,
                                                     int* __restrict__ flag)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool open = false;
    if (i < n) {
        if (merge && contrib[4 * n + i] != 0) {
#pragma unroll
            for (int p = 0; p < 5; ++p) state[p * n + i] = contrib[p * n + i];
        }
        const float status = __int_as_float(state[3 * n + i]);
        open = status == 0.0f || status == 3.0f;
    }
    if (__ballot(open) != 0ull && threadIdx.x % 64 == 0) atomicOr(flag, 1);
}

// ---- exact march, hand-over protocol (kfx_slab_raycast_exact) --------------------------------------------------------
// A ray's march state travels with the ray: after a rank has marched its segment the state goes to the two neighbour ranks
// only (planes 0-4 as they are: nothing is compacted, the receiver picks the rays that came its way), and a rank adopts from
// a neighbour's planes the rays that neighbour advanced in this stage and that are still under way (status 0: marching, 3:
// hit found, normal pending).  No rank ever acts on a stale copy: k_raycast_sdf_slab advances a ray only while the trilinear
// base plane of its current sample is one the rank owns, a ray moves through the planes monotonically, so the plane of a
// stale position belongs to a rank the ray has left -- and that rank holds the newer state.
// fin[i] = this rank finalised pixel i (set its status to 1 hit / 2 miss), the one rank whose result counts at the end.
__global__ __launch_bounds__(256) void k_handover_merge(int* __restrict__ state, const int* __restrict__ from_lo, const int* __restrict__ from_hi,
                                                        int* __restrict__ fin, size_t n, int claim_untouched_misses)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool touched = state[4 * n + i] != 0;
    const float status = __int_as_float(state[3 * n + i]);
    if (touched && (status == 1.0f || status == 2.0f)) fin[i] = 1;
    // rays that never enter the box are misses from the first stage on, on every rank alike: rank 0 answers for them
    if (claim_untouched_misses && !touched && status == 2.0f) fin[i] = 1;
    const int* src = nullptr;
    if (from_lo && from_lo[4 * n + i] != 0) {
        const float st = __int_as_float(from_lo[3 * n + i]);
        if (st == 0.0f || st == 3.0f) src = from_lo;
    }
    if (!src && from_hi && from_hi[4 * n + i] != 0) {
        const float st = __int_as_float(from_hi[3 * n + i]);
        if (st == 0.0f || st == 3.0f) src = from_hi;
    }
    if (src) {
#pragma unroll
        for (int p = 0; p < 4; ++p) state[p * n + i] = src[p * n + i];
    }
}

// contribution of this rank to the final images: lambda, status, normal, shade of the pixels it finalised, zero elsewhere
// (integer bit patterns: NaN and -0 survive the SUM over ranks, where exactly one rank is non-zero)
__global__ __launch_bounds__(256) void k_handover_contrib(const int* __restrict__ state, const int* __restrict__ fin, int* __restrict__ contrib, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool mine = fin[i] != 0;
    contrib[0 * n + i] = mine ? state[0 * n + i] : 0;
    contrib[1 * n + i] = mine ? state[3 * n + i] : 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) contrib[(2 + p) * n + i] = mine ? state[(5 + p) * n + i] : 0;
}

// the summed contributions back into the state; *open += pixels without a final status (none, unless the protocol is broken)
__global__ __launch_bounds__(256) void k_handover_finish(int* __restrict__ state, const int* __restrict__ contrib, size_t n, int* __restrict__ open)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) {
        state[0 * n + i] = contrib[0 * n + i];
        state[3 * n + i] = contrib[1 * n + i];
#pragma unroll
        for (int p = 0; p < 4; ++p) state[(5 + p) * n + i] = contrib[(2 + p) * n + i];
        const float status = __int_as_float(contrib[1 * n + i]);
        bad = !(status == 1.0f || status == 2.0f);
    }
    const unsigned long long m = __ballot(bad);
    if (m != 0ull && threadIdx.x % 64 == 0) atomicAdd(open, __popcll(m));   // (a wave's first thread adds the wave's count)
}

// ---- tile-pipelined hand-over (kfx_slab_raycast_exact_tiled) ---------------------------------------------------------
// State per row-tile t (kfx.h, kfx_raycast_sdf_slab_tiles): NP march planes at M + (t * NP + k) * P -- the token of a tile --, results
// at Rz + (t * 4 + k) * P.  NP = 3, packed {lambda, last_sdf, delta of a marching ray or -status}: 12 B per pixel ("12 B
// per ray of march state"), whenever the truncation distance is positive; else the four planes {lambda, last_sdf, delta, status}.
// "Newer wins": a ray's copies on different ranks are snapshots of ONE march; status 1 / 2 (final) is later than 3 (hit, normal
// pending) is later than 0 (marching), and of two marching snapshots the one with the larger lambda is later (every step adds a
// positive delta).  A rank never advances a stale copy -- it advances a ray only while the base plane of its current sample is
// one it owns, and a kernel run leaves no marching ray of the tile inside the rank's own planes -- so adopting the neighbour's
// newer, still-open snapshot is all the merging there is; k_raycast_sdf_slab does it at the start of a visit (raycast.hip).

// Where word c of pixel i of the six result planes {lambda, status, n.x, n.y, n.z, shade} lives: dense [6][n] (S = 0), or by image
// strips (S = pixels per strip, kfx_composite_strip_pixels): strip j = pixels [j S, (j + 1) S) of the row-major image holds its six
// planes side by side at (j * 6 + c) * S -- the layout in which strip j travels to its owner rank j and back.
__device__ __forceinline__ size_t result_index(int c, size_t i, size_t n, unsigned S)
{
    if (S == 0) return (size_t)c * n + i;
    const size_t j = i / S;
    return (j * 6 + (size_t)c) * S + (i - j * S);
}

// this rank's contribution to the final images: lambda, status, normal, shade of the pixels it finalised, zero elsewhere (integer
// bit patterns: NaN and -0 survive the sum over ranks, of which exactly one is non-zero per pixel)
__global__ __launch_bounds__(256) void k_tiles_contrib(const int* __restrict__ M, const int* __restrict__ Rz, const int* __restrict__ fin,
                                                       int* __restrict__ contrib, int w, int h, int R, size_t P, unsigned S, int packed)
{
    int u, v;
    pixel_xy(u, v);
    if (u >= w || v >= h) return;
    const size_t n = (size_t)w * h, i = (size_t)v * w + u;
    const int t = v / R;
    const size_t q = (size_t)(v - t * R) * w + u;
    const int* st = M + (size_t)t * (packed ? 3 : 4) * P + q;
    const int* rs = Rz + (size_t)t * 4 * P + q;
    const bool mine = fin[i] != 0;
    contrib[result_index(0, i, n, S)] = mine ? st[0] : 0;
    int status = 0;   // the status plane's bits: a finalised ray's 1.0f / 2.0f
    if (mine) {
        if (packed) { const float c = __int_as_float(st[2 * P]); status = __float_as_int(c < 0.f ? -c : 0.f); }
        else status = st[3 * P];
    }
    contrib[result_index(1, i, n, S)] = status;
#pragma unroll
    for (int k = 0; k < 4; ++k) contrib[result_index(2 + k, i, n, S)] = mine ? rs[k * P] : 0;
}

// the owner of a strip adds up the ranks' copies of it: in + r * 6 * S = rank r's [6][S]; out [6][S]
__global__ __launch_bounds__(256) void k_strip_sum(const int* __restrict__ in, int* __restrict__ out, size_t words, int world)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    int acc = 0;
    for (int r = 0; r < world; ++r) acc += in[(size_t)r * words + i];
    out[i] = acc;
}

// the summed contributions -> depth / normal / shade images (cu_raycast.cu:92-108: a miss is NaN, a zero normal, a zero shade);
// *open += pixels without a final status
__global__ __launch_bounds__(256) void k_tiles_finish(const RenderImages im, const int* __restrict__ contrib, int* __restrict__ open, unsigned S)
{
    int u, v;
    pixel_xy(u, v);
    bool bad = false;
    if (u < im.w && v < im.h) {
        const size_t n = (size_t)im.w * im.h, i = (size_t)v * im.w + u;
        const auto word = [&](int c) { return __int_as_float(contrib[result_index(c, i, n, S)]); };
        const float depth = word(0), status = word(1);
        bad = !(status == 1.0f || status == 2.0f);
        const RayOut o = ray_out(im, u, v);
        if (status == 1.0f && depth > 0.0f) write_hit(o, depth, make_float4(word(2), word(3), word(4), 1.0f), word(5));
        else write_no_hit(o);
    }
    const unsigned long long m = __ballot(bad);
    if (m != 0ull && threadIdx.x % 64 == 0) atomicAdd(open, __popcll(m));   // (a wave's first thread adds the wave's count)
}

} // namespace kfx

using namespace kfx;

extern "C" int kfx_slab_layout_init(kfx_slab_layout* L, size_t full_d, float full_zmin, float full_zmax, int rank, int world, int ghost)
{
    if (!L) return set_error(KFX_E_NULL, "kfx_slab_layout_init: null layout");
    if (full_d < 2 || world < 1 || rank < 0 || rank >= world || ghost < 1 || (size_t)world > full_d)
        return set_error(KFX_E_RANGE, "kfx_slab_layout_init: need full_d >= 2, 0 <= rank < world <= full_d, ghost >= 1");
    const size_t base = full_d / (size_t)world, rem = full_d % (size_t)world;
    if (world > 1 && base < (size_t)ghost) return set_error(KFX_E_RANGE, "kfx_slab_layout_init: every rank must own at least `ghost` planes");
    L->full_d = full_d;
    L->full_zmin = full_zmin;
    L->full_zmax = full_zmax;
    L->rank = rank;
    L->world = world;
    L->ghost = ghost;
    const size_t r = (size_t)rank;
    L->z0 = r * base + (r < rem ? r : rem);
    L->z1 = L->z0 + base + (r < rem ? 1 : 0);
    L->s0 = L->z0 >= (size_t)ghost ? L->z0 - (size_t)ghost : 0;
    L->s1 = L->z1 + (size_t)ghost <= full_d ? L->z1 + (size_t)ghost : full_d;
    // BoundedVolume::VoxelPositionInUnits (BoundedVolume.h:115-125): min + size * i / (float)(d - 1)
    const float size_z = full_zmax - full_zmin;
    L->local_zmin = full_zmin + size_z * (float)L->s0 / (float)(full_d - 1);
    L->local_zmax = full_zmin + size_z * (float)(L->s1 - 1) / (float)(full_d - 1);
    return 0;
}

extern "C" int kfx_slab_broadcast_inputs(const kfx_image* depth, const kfx_image* norm, void* scratch, int root, kfx_comm* comm, kfx_stream stream)
{
    if (!comm) return set_error(KFX_E_NULL, "kfx_slab_broadcast_inputs: null argument");
    if (int e = check_image(depth, 4, 0, 0, "kfx_slab_broadcast_inputs: depth image")) return e;
    if (int e = check_image(norm, 16, 0, 0, "kfx_slab_broadcast_inputs: normal image")) return e;
    if (norm->w != depth->w || norm->h != depth->h) return set_error(KFX_E_SHAPE, "kfx_slab_broadcast_inputs: depth and normals differ in size");
    if (comm->world == 1) return 0;
    if (!comm->broadcast) return set_error(KFX_E_NULL, "kfx_slab_broadcast_inputs: the transport has no broadcast");
    const size_t w = depth->w, h = depth->h;
    if (w == 0 || h == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool dense = depth->pitch == w * 4 && norm->pitch == w * 16;
    if (dense) {
        if (int e = comm->broadcast(comm, depth->ptr, w * h * 4, root, stream)) return e;
        return comm->broadcast(comm, norm->ptr, w * h * 16, root, stream);
    }
    if (!scratch) return set_error(KFX_E_NULL, "kfx_slab_broadcast_inputs: pitched images need the scratch buffer");
    unsigned char* sd = static_cast<unsigned char*>(scratch);
    unsigned char* sn = sd + w * h * 4;
    if (comm->rank == root) {
        if (int e = hip_status(hipMemcpy2DAsync(sd, w * 4, depth->ptr, depth->pitch, w * 4, h, hipMemcpyDeviceToDevice, s), "kfx_slab_broadcast_inputs")) return e;
        if (int e = hip_status(hipMemcpy2DAsync(sn, w * 16, norm->ptr, norm->pitch, w * 16, h, hipMemcpyDeviceToDevice, s), "kfx_slab_broadcast_inputs")) return e;
    }
    if (int e = comm->broadcast(comm, sd, w * h * 20, root, stream)) return e;
    if (comm->rank != root) {
        if (int e = hip_status(hipMemcpy2DAsync(depth->ptr, depth->pitch, sd, w * 4, w * 4, h, hipMemcpyDeviceToDevice, s), "kfx_slab_broadcast_inputs")) return e;
        if (int e = hip_status(hipMemcpy2DAsync(norm->ptr, norm->pitch, sn, w * 16, w * 16, h, hipMemcpyDeviceToDevice, s), "kfx_slab_broadcast_inputs")) return e;
    }
    return 0;
}

extern "C" int kfx_slab_exchange_halos(const kfx_volume* local, const kfx_slab_layout* L, kfx_comm* comm, kfx_stream stream)
{
    if (!local || !local->ptr || !L || !comm) return set_error(KFX_E_NULL, "kfx_slab_exchange_halos: null argument");
    if (int e = check_layout(local, L, comm, "kfx_slab_exchange_halos")) return e;
    if (L->world == 1) return 0;
    unsigned char* base = static_cast<unsigned char*>(local->ptr);
    const size_t plane = local->img_pitch;
    const size_t lo_ghost = L->z0 - L->s0, hi_ghost = L->s1 - L->z1;   // planes [s0, z0) come from rank - 1, [z1, s1) from rank + 1
    const size_t own0 = L->z0 - L->s0, own1 = L->z1 - L->s0;           // local indices of the owned range
    // the lower neighbour's upper ghost is `ghost` planes unless it is clipped by the volume's end -- it never is for
    // rank - 1 < world - 1; symmetric for the upper neighbour: both directions carry lo_ghost / hi_ghost planes
    const bool lo = L->rank > 0, hi = L->rank + 1 < L->world;
    // my first owned planes -> rank - 1's upper ghost, my last owned planes -> rank + 1's lower ghost
    return comm->exchange(comm, lo ? base + own0 * plane : nullptr, lo ? base : nullptr, lo ? lo_ghost * plane : 0,
                          hi ? base + (own1 - hi_ghost) * plane : nullptr, hi ? base + own1 * plane : nullptr, hi ? hi_ghost * plane : 0, stream);
}

extern "C" int kfx_slab_composite(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, long long* key, float* payload,
                                  kfx_comm* comm, kfx_stream stream)
{
    if (!comm || !depth) return set_error(KFX_E_NULL, "kfx_slab_composite: null argument");
    if (comm->world == 1) return 0;
    const size_t n = depth->w * depth->h;
    if (int e = kfx_composite_pack(depth, norm, img, key, comm->rank, stream)) return e;
    if (int e = comm->all_reduce(comm, key, n, KFX_COMM_MIN_I64, stream)) return e;
    if (int e = kfx_composite_select(depth, norm, img, key, payload, comm->rank, stream)) return e;
    if (int e = comm->all_reduce(comm, payload, KFX_COMPOSITE_PAYLOAD * n, KFX_COMM_SUM_F32, stream)) return e;
    return kfx_composite_unpack(depth, norm, img, key, payload, stream);
}

extern "C" size_t kfx_slab_composite_direct_scratch_bytes(size_t w, size_t h, int world)
{
    if (world < 1) return 0;   // send strips, received / gathered strips, this rank's merged strip
    return (2 * (size_t)world + 1) * KFX_COMPOSITE_STRIP_PLANES * kfx_composite_strip_pixels(w, h, world) * sizeof(float);
}

extern "C" int kfx_slab_composite_direct(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, void* scratch, kfx_comm* comm,
                                         kfx_stream stream)
{
    if (!comm || !depth) return set_error(KFX_E_NULL, "kfx_slab_composite_direct: null argument");
    if (comm->world == 1) return 0;
    // argument errors every rank makes alike come back before any collective; a LOCAL failure from here on: FirstError
    if (!scratch) return set_error(KFX_E_NULL, "kfx_slab_composite_direct: null scratch");
    if (!comm->all_to_all || !comm->all_gather) return set_error(KFX_E_RANGE, "kfx_slab_composite_direct: the transport has no all_to_all / all_gather");
    const int W = comm->world;
    const size_t S = kfx_composite_strip_pixels(depth->w, depth->h, W), strip = KFX_COMPOSITE_STRIP_PLANES * S;
    float* send = static_cast<float*>(scratch);
    float* recv = send + (size_t)W * strip;
    float* merged = recv + (size_t)W * strip;
    FirstError note;
    note(kfx_composite_strips_pack(depth, norm, img, send, 0, W, stream));
    note(comm->all_to_all(comm, send, recv, strip * sizeof(float), stream));
    note(kfx_composite_strips_merge(recv, merged, S, 0, W, stream));
    note(comm->all_gather(comm, merged, recv, strip * sizeof(float), stream));
    return note.status ? note.status : kfx_composite_strips_unpack(depth, norm, img, recv, 0, W, stream);
}

extern "C" size_t kfx_slab_exact_scratch_bytes(size_t w, size_t h) { return (17 * w * h + 64) * sizeof(int); }

static int exact_args(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, float* state, void* scratch,
                      const kfx_volume* local, const kfx_slab_layout* L, kfx_comm* comm, const char* who)
{
    if (!depth || !norm || !img || !state || !scratch || !local || !L || !comm) return set_error(KFX_E_NULL, who);
    if (int e = check_layout(local, L, comm, "kfx_slab_raycast_exact")) return e;
    return check_render_images(depth, norm, img, img, "kfx_slab_raycast_exact");   // (what kfx_raycast_state_to_images asks at the end)
}

// The blueprint's hand-over: world + 1 march stages with a neighbour exchange of the march planes between
// them -- a ray that enters at one end needs `world` stages to reach the other, one more lets a hit on a slab boundary have
// its normal evaluated by the neighbour that owns the gradient's base plane --, then ONE all-reduce of the finalising ranks'
// results and ONE read-back (the count of rays without a final status: zero).  No host synchronisation between the stages.
extern "C" int kfx_slab_raycast_exact(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, float* state, void* scratch,
                                      const kfx_volume* local, const kfx_slab_layout* L, const float T_wc[12], const float K[4],
                                      float near, float far, float trunc_dist, int subpix, kfx_comm* comm, kfx_stream stream,
                                      int* rounds_out)
{
    if (int e = exact_args(depth, norm, img, state, scratch, local, L, comm, "kfx_slab_raycast_exact: null argument")) return e;
    const int w = (int)depth->w, h = (int)depth->h;
    const size_t n = (size_t)w * h;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int* from_lo = static_cast<int*>(scratch);
    int* from_hi = from_lo + 5 * n;
    int* fin = from_hi + 5 * n;
    int* contrib = fin + n;
    int* open = contrib + 6 * n;
    int* istate = reinterpret_cast<int*>(state);
    const kfx_slab slab = {L->full_d, L->s0, L->full_zmin, L->full_zmax};
    const dim3 grid((unsigned)((n + 255) / 256));
    const int world = comm->world, rank = comm->rank;
    const int stages = world > 1 ? world + 1 : 1;
    FirstError note;   // (no early return between the collectives)
    if (world > 1) note(hip_status(hipMemsetAsync(fin, 0, (7 * n + 1) * sizeof(int), s), "kfx_slab_raycast_exact")); // fin, contrib, open
    for (int stage = 0; stage < stages; ++stage) {
        note(kfx_raycast_sdf_slab(state, stage == 0, local, &slab, (int)L->z0, (int)L->z1, w, h, T_wc, K, near, far, trunc_dist, subpix, stream));
        if (world == 1) break;
        const bool exchange = stage + 1 < stages;
        if (exchange) note(comm->exchange(comm, istate, from_lo, 5 * n * sizeof(int), istate, from_hi, 5 * n * sizeof(int), stream));
        hipLaunchKernelGGL(k_handover_merge, grid, dim3(256), 0, s, istate, (exchange && rank > 0) ? from_lo : nullptr,
                           (exchange && rank + 1 < world) ? from_hi : nullptr, fin, n, (stage == 0 && rank == 0) ? 1 : 0);
        note(check_launch("kfx_slab_raycast_exact"));
    }
    if (world > 1) {
        hipLaunchKernelGGL(k_handover_contrib, grid, dim3(256), 0, s, istate, fin, contrib, n);
        note(check_launch("kfx_slab_raycast_exact"));
        note(comm->all_reduce(comm, contrib, 6 * n, KFX_COMM_SUM_I32, stream));
        hipLaunchKernelGGL(k_handover_finish, grid, dim3(256), 0, s, istate, contrib, n, open);
        note(check_launch("kfx_slab_raycast_exact"));
        int n_open = 0;
        note(hip_status(hipMemcpyAsync(&n_open, open, sizeof(int), hipMemcpyDeviceToHost, s), "kfx_slab_raycast_exact"));
        note(hip_status(hipStreamSynchronize(s), "kfx_slab_raycast_exact"));   // the frame's one synchronisation
        if (!note.status && n_open) note(set_error(KFX_E_RANGE, "kfx_slab_raycast_exact: rays without a final status after world + 1 stages"));
    }
    if (rounds_out) *rounds_out = stages;
    return note.status ? note.status : kfx_raycast_state_to_images(depth, norm, img, state, stream);
}

// The cross-check of the hand-over: rounds of kfx_raycast_sdf_slab with one SUM all-reduce of the touched pixels' march state
// per round (every rank always holds every ray's state) and a host-side termination test after each -- <= world + 2 rounds,
// each a host synchronisation.  Same images, bit for bit.
extern "C" int kfx_slab_raycast_exact_allreduce(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, float* state, void* scratch,
                                      const kfx_volume* local, const kfx_slab_layout* L, const float T_wc[12], const float K[4],
                                      float near, float far, float trunc_dist, int subpix, kfx_comm* comm, kfx_stream stream,
                                      int* rounds_out)
{
    if (int e = exact_args(depth, norm, img, state, scratch, local, L, comm, "kfx_slab_raycast_exact_allreduce: null argument")) return e;
    const int w = (int)depth->w, h = (int)depth->h;
    const size_t n = (size_t)w * h;
    if (n == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    int* contrib = static_cast<int*>(scratch);
    int* flag = contrib + 5 * n;
    int* istate = reinterpret_cast<int*>(state);
    const kfx_slab slab = {L->full_d, L->s0, L->full_zmin, L->full_zmax};
    const dim3 grid((unsigned)((n + 255) / 256));
    int rounds = 0;
    for (;;) {
        if (int e = kfx_raycast_sdf_slab(state, rounds == 0, local, &slab, (int)L->z0, (int)L->z1, w, h, T_wc, K, near, far,
                                         trunc_dist, subpix, stream))
            return e;
        ++rounds;
        if (comm->world > 1) {
            hipLaunchKernelGGL(k_state_contrib, grid, dim3(256), 0, s, istate, contrib, n);
            if (int e = check_launch("kfx_slab_raycast_exact")) return e;
            if (int e = comm->all_reduce(comm, contrib, 5 * n, KFX_COMM_SUM_I32, stream)) return e;
        }
        if (int e = hip_status(hipMemsetAsync(flag, 0, sizeof(int), s), "kfx_slab_raycast_exact")) return e;
        hipLaunchKernelGGL(k_state_merge, grid, dim3(256), 0, s, istate, contrib, n, comm->world > 1 ? 1 : 0, flag);
        if (int e = check_launch("kfx_slab_raycast_exact")) return e;
        int open = 0;
        if (int e = hip_status(hipMemcpyAsync(&open, flag, sizeof(int), hipMemcpyDeviceToHost, s), "kfx_slab_raycast_exact")) return e;
        if (int e = hip_status(hipStreamSynchronize(s), "kfx_slab_raycast_exact")) return e;
        if (!open) break; // the merged state is identical on every rank, so all ranks leave together
        if (rounds > L->world + 3) return set_error(KFX_E_RANGE, "kfx_slab_raycast_exact: march did not terminate");
    }
    if (comm->world > 1) // normals (planes 5-7) and shade (8): written by one rank per pixel
        if (int e = comm->all_reduce(comm, istate + 5 * n, 4 * n, KFX_COMM_SUM_I32, stream)) return e;
    if (rounds_out) *rounds_out = rounds;
    return kfx_raycast_state_to_images(depth, norm, img, state, stream);
}

// ---- the hand-over pipelined over image row-tiles (kfx_slab.h) -------------------------------------------------------------
// One set of the final exchange's buffers carved out of `mem` (null: sizes only); returns its size in ints.  Dense [6][n] for the
// all-reduce (and for one rank), by strips [world][6][S] for the direct sends.
size_t kfx::exact_final_carve(ExactFinalBufs& b, void* mem, size_t w, size_t h, int world)
{
    if (world < 1) world = 1;
    const size_t n = w * h;
    b.S = world > 1 ? kfx_composite_strip_pixels(w, h, world) : 0;
    const size_t by_strips = (size_t)(world > 1 ? world : 0) * 6 * b.S;
    int* base = static_cast<int*>(mem);
    size_t o = 0;
    const auto take = [&](size_t ints) { int* q = base ? base + o : nullptr; o += (ints + 63) / 64 * 64; return q; };
    b.contrib = take(by_strips > 6 * n ? by_strips : 6 * n);
    b.gathered = take(by_strips);
    b.mine = take(6 * b.S);
    b.open = take(64);
    return o;
}

// the scratch buffer's parts; returns its size in ints (scratch may be null: sizes only)
size_t kfx::tiled_layout(TiledScratch& t, void* scratch, size_t w, size_t h, int tiles, int world)
{
    if (tiles > 64) tiles = 64;   // (the march keeps a 64-bit mask of the tiles it has initialised; clamped HERE so that the advertised size and the march agree)
    t.T = tiles < 1 ? 1 : (tiles > (int)h ? (int)(h ? h : 1) : tiles);
    t.R = (int)((h + (size_t)t.T - 1) / (size_t)t.T);
    t.T = (int)((h + (size_t)t.R - 1) / (size_t)(t.R ? t.R : 1));   // (tiles that are not empty)
    t.P = ((size_t)t.R * w + 63) / 64 * 64;
    t.n = w * h;
    int* base = static_cast<int*>(scratch);
    size_t o = 0;
    const auto take = [&](size_t ints) { int* q = base ? base + o : nullptr; o += ints; return q; };
    t.M = take((size_t)t.T * 4 * t.P);
    t.Rz = take((size_t)t.T * 4 * t.P);
    t.from_lo = take((size_t)t.T * 4 * t.P);
    t.from_hi = take((size_t)t.T * 4 * t.P);
    t.fin = take((t.n + 63) / 64 * 64);
    return o + exact_final_carve(t.own, base ? base + o : nullptr, w, h, world);
}

// the final exchange goes by direct sends over the mesh unless KFX_SLAB_FINALISE=allreduce asks for the all-reduce or the transport lacks them
static bool finalise_direct(const kfx_comm* comm)
{
    static const bool by_allreduce = env_begins("KFX_SLAB_FINALISE", "a");
    return comm->world > 1 && !by_allreduce && comm->all_to_all && comm->all_gather;
}

extern "C" size_t kfx_slab_exact_tiled_scratch_bytes(size_t w, size_t h, int tiles, int world)
{
    if (w == 0 || h == 0) return 256;
    TiledScratch t;
    return tiled_layout(t, nullptr, w, h, tiles, world < 1 ? 1 : world) * sizeof(int);
}

// The image's four corner rays through K, ((u - u0) / fu, (v - v0) / fv, 1) at u in {0, w - 1}, v in {0, h - 1}: f(cx, cy) for each.
// What is affine in the pixel -- a ray's z-direction -- or convex in it -- its length -- takes its extremes there.
template <typename F>
static void for_corner_rays(const float K[4], int w, int h, const F& f)
{
    for (int c = 0; c < 4; ++c) {
        const double cx = ((c & 1 ? (double)(w - 1) : 0.0) - (double)K[2]) / (double)K[0], cy = ((c & 2 ? (double)(h - 1) : 0.0) - (double)K[3]) / (double)K[1];
        f(cx, cy);
    }
}

// Ghost planes per side with which the exact hand-over needs no last stage for the normals.  A hit is found at a sample whose base
// plane the finder owns; its sub-step interpolation (cu_raycast.cu:70-74) puts it at most one step behind that sample, a step is at
// most max(trunc_dist, voxel.x) (the march's step is the sampled value, and a TSDF's cells do not exceed the truncation distance:
// Sdf.h, cu_sdffusion.cu:49), a ray moves |ray| <= the longest ((u - u0) / fu, (v - v0) / fv, 1) of the image per unit of lambda;
// the gradient stencil (Volume.h:262-289) takes one plane below and one above its base plane.
extern "C" int kfx_slab_exact_ghost(size_t full_d, float full_zmin, float full_zmax, float size_x, size_t vol_w, float trunc_dist, const float K[4], int w, int h)
{
    if (!K || full_d < 2 || vol_w < 2 || w < 1 || h < 1) return 2;
    const double vz = std::fabs(((double)full_zmax - (double)full_zmin) / (double)(full_d - 1)), vx = std::fabs((double)size_x / (double)(vol_w - 1));
    double rmax = 1.0;
    for_corner_rays(K, w, h, [&](double cx, double cy) {
        const double r = std::sqrt(cx * cx + cy * cy + 1.0);
        rmax = r > rmax ? r : rmax;
    });
    const double step = (double)trunc_dist > vx ? (double)trunc_dist : vx;
    const double planes = rmax * step / vz;
    if (!(trunc_dist > 0.f) || !(vz > 0.0) || !(planes < 1e6)) return 2;   // (degenerate: the ordinary width, with the last stage)
    return (int)std::ceil(planes * 1.001 + 0.01) + 2;
}

namespace {
std::atomic<int> g_normals_stage{-1};   // -1: not read yet (KFX_SLAB_NORMALS_STAGE, default 0)
bool normals_stage_forced()
{
    int v = g_normals_stage.load(std::memory_order_relaxed);
    if (v < 0) {
        v = env_int("KFX_SLAB_NORMALS_STAGE", 0) != 0 ? 1 : 0;
        g_normals_stage.store(v, std::memory_order_relaxed);
    }
    return v != 0;
}
} // namespace

// 1: the hand-over keeps its last stage whatever the layout's ghost width (measurements, cross-checks; every rank alike); 0: dropped
// where the ghost planes allow.  Returns the previous setting.
extern "C" int kfx_slab_set_normals_stage(int keep)
{
    const int prev = normals_stage_forced() ? 1 : 0;
    g_normals_stage.store(keep ? 1 : 0, std::memory_order_relaxed);
    return prev;
}

// The march: token steps, the normals' stage, and this rank's contribution to the final images left in `fb`.  Everything here is
// ordered on `stream`; the collectives are neighbour exchanges only (comm->exchange_v).
int kfx::exact_tiled_march(const TiledScratch& t, const ExactFinalBufs& fb, const kfx_volume* local, const kfx_slab_layout* L, const float T_wc[12],
                           const float K[4], float near, float far, float trunc_dist, int subpix, int w, int h, kfx_comm* comm, kfx_stream stream,
                           int* steps_out, const kfx_volume* color_local)
{
    const int world = comm->world, rank = comm->rank;
    const int T = t.T, R = t.R;
    // the tile state packed into three planes (12 B per pixel and hop) unless a marching ray's delta could be negative; every rank
    // decides alike from the same arguments
    const int packed = trunc_dist > 0.f ? 1 : 0, NP = packed ? 3 : 4;
    const size_t P = t.P, tile_bytes = (size_t)NP * P * sizeof(int);
    // With ghost planes as wide as a hit can fall back behind the sample that found it (kfx_slab_exact_ghost), the rank that finds a
    // hit always holds its gradient stencil: it finalises the hit itself and the hand-over needs no last stage for the normals
    const int self_normals = (world > 1 && L->ghost >= kfx_slab_exact_ghost(L->full_d, L->full_zmin, L->full_zmax, local->boxmax[0] - local->boxmin[0],
                                                                          (size_t)local->w, trunc_dist, K, w, h) && !normals_stage_forced()) ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const kfx_slab slab = {L->full_d, L->s0, L->full_zmin, L->full_zmax};
    FirstError note;   // (no early return between the collectives)
    // one launch per visit of a tile: it initialises the tile's rays when this is the rank's first visit, takes over what the
    // neighbours handed on (their newer, still open snapshots), and marches what lies in the rank's own planes
    auto march = [&](int v0, int v1, int init, const int* from_lo, const int* from_hi, int tile_major) {
        const int layout_flags = (tile_major ? 1 : 0) | (packed ? 2 : 0) | (self_normals ? 4 : 0);
        if (color_local)
            note(kfx_raycast_sdf_slab_tiles_color(reinterpret_cast<float*>(t.M), reinterpret_cast<float*>(t.Rz), P, R, v0, v1, init, t.fin, rank == 0 ? 1 : 0,
                                                  reinterpret_cast<const float*>(from_lo), reinterpret_cast<const float*>(from_hi), layout_flags, local, color_local,
                                                  &slab, (int)L->z0, (int)L->z1, w, h, T_wc, K, near, far, trunc_dist, subpix, stream));
        else
            note(kfx_raycast_sdf_slab_tiles(reinterpret_cast<float*>(t.M), reinterpret_cast<float*>(t.Rz), P, R, v0, v1, init, t.fin, rank == 0 ? 1 : 0,
                                            reinterpret_cast<const float*>(from_lo), reinterpret_cast<const float*>(from_hi), layout_flags, local, &slab,
                                            (int)L->z0, (int)L->z1, w, h, T_wc, K, near, far, trunc_dist, subpix, stream));
    };
    unsigned long long seen = 0ull;   // tiles this rank has initialised (tiles <= 64)
    auto visit = [&](int tile, const int* from_lo, const int* from_hi) {   // the tile's rows, initialised at the rank's first visit
        const int v0 = tile * R;
        march(v0, v0 + R < h ? v0 + R : h, (seen >> tile) & 1ull ? 0 : 1, from_lo, from_hi, 0);
        seen |= 1ull << tile;
    };
    int steps = 0;
    if (world == 1) {
        march(0, h, 1, nullptr, nullptr, 0);
        steps = 1;
    } else {
        // Every rank starts every ray itself, tile by tile at its first visit (the entry slab's owner is the one that can advance
        // it).  Rank r visits tile t when the upward token reaches it (step r + t) and when the downward one does (W - 1 - r + t).
        // Which tokens exist: a ray's z-direction is R_wc's third row against ((u - u0) / fu, (v - v0) / fv, 1) -- affine in the
        // pixel, so its extremes sit in the image's corners.  When every ray rises (the usual case: the camera looks along the
        // slabs' axis) nothing ever travels downwards -- no downward visits, no downward messages -- and the normals' stage sends
        // downwards only (a rising ray's hit falls BACK across a boundary); likewise for all-falling rays.  Every rank derives the
        // same two flags from the same pose (with a margin: rays that are flat within it count as both).
        bool need_up = true, need_down = true;
        {
            double zlo = 1e300, zhi = -1e300, mag = 0.0;
            for_corner_rays(K, w, h, [&](double cx, double cy) {
                const double z = (double)T_wc[8] * cx + (double)T_wc[9] * cy + (double)T_wc[10];
                const double m = std::fabs((double)T_wc[8] * cx) + std::fabs((double)T_wc[9] * cy) + std::fabs((double)T_wc[10]);
                zlo = z < zlo ? z : zlo; zhi = z > zhi ? z : zhi; mag = m > mag ? m : mag;
            });
            const double margin = 1e-4 * mag;
            if (zlo == zlo && zhi == zhi && mag < 1e300) {   // (a pose with NaN keeps both)
                need_down = !(zlo > margin);
                need_up = !(zhi < -margin);
            }
        }
        bool got_lo = false, got_hi = false;   // what the previous step's exchange brought: tile A (from below) / tile B (from above) of THIS step
        for (int d = 0; d < world + T - 1; ++d, ++steps) {
            const int A = d - rank, B = d - (world - 1 - rank);   // the tiles the upward / downward token brings to this rank now
            const bool a_ok = need_up && A >= 0 && A < T, b_ok = need_down && B >= 0 && B < T;
            if (a_ok) visit(A, got_lo ? t.from_lo : nullptr, (b_ok && B == A && got_hi) ? t.from_hi : nullptr);
            if (b_ok && !(a_ok && B == A)) visit(B, nullptr, got_hi ? t.from_hi : nullptr);
            // pass the tokens on: tile A upwards, tile B downwards; what arrives is the tile this rank marches in the next step
            const bool up = a_ok && rank + 1 < world, down = b_ok && rank > 0;
            const bool from_below = need_up && rank > 0 && A + 1 >= 0 && A + 1 < T, from_above = need_down && rank + 1 < world && B + 1 >= 0 && B + 1 < T;
            // (every rank calls the exchange in every step, with empty legs where it has nothing to pass on: a transport may
            //  synchronise its ranks inside the call, as the in-process one does in its barrier mode)
            note(comm->exchange_v(comm, down ? t.M + (size_t)B * NP * P : nullptr, down ? tile_bytes : 0, from_below ? t.from_lo : nullptr, from_below ? tile_bytes : 0,
                                  up ? t.M + (size_t)A * NP * P : nullptr, up ? tile_bytes : 0, from_above ? t.from_hi : nullptr, from_above ? tile_bytes : 0, stream));
            got_lo = from_below; got_hi = from_above;
        }
        // one more stage over the whole image: a hit whose sub-step interpolation fell back across a slab boundary has its normal
        // evaluated by the neighbour that owns the gradient's base plane -- the one BEHIND the ray: rising rays' hits go down, falling
        // rays' up
        // (not with ghost planes wide enough for every finder to finalise its own hits: self_normals.  A ray left without a final
        //  status -- cells beyond the truncation distance -- is counted by the final exchange and reported: KFX_E_RANGE)
        if (!self_normals) {
            const size_t all = (size_t)T * tile_bytes;
            const bool send_down = need_up && rank > 0, recv_from_above = need_up && rank + 1 < world;       // rising rays' pending normals
            const bool send_up = need_down && rank + 1 < world, recv_from_below = need_down && rank > 0;     // falling rays'
            note(comm->exchange_v(comm, send_down ? t.M : nullptr, send_down ? all : 0, recv_from_below ? t.from_lo : nullptr, recv_from_below ? all : 0,
                                  send_up ? t.M : nullptr, send_up ? all : 0, recv_from_above ? t.from_hi : nullptr, recv_from_above ? all : 0, stream));
            march(0, h, 0, recv_from_below ? t.from_lo : nullptr, recv_from_above ? t.from_hi : nullptr, 1);
            ++steps;
        }
    }
    // Every pixel has been given its final status by exactly one rank: this rank's contribution to the final images, in the layout of
    // the exchange that follows (exact_tiled_finalise)
    const bool direct = finalise_direct(comm);
    const unsigned S = direct ? (unsigned)fb.S : 0u;
    if (direct && (size_t)world * fb.S > t.n)   // the last strip's padding travels too: defined (and summed as zero)
        note(hip_status(hipMemsetAsync(fb.contrib + ((size_t)(world - 1) * 6) * fb.S, 0, 6 * fb.S * sizeof(int), s), "kfx_slab_raycast_exact_tiled"));
    hipLaunchKernelGGL(k_tiles_contrib, pixel_grid(w, h), dim3(256), 0, s, t.M, t.Rz, t.fin, fb.contrib, w, h, R, P, S, packed);
    note(check_launch("kfx_slab_raycast_exact_tiled"));
    if (steps_out) *steps_out = steps;   // world + tiles - 1 token steps + the normals' stage (1 for a single rank)
    return note.status;
}

// The final exchange.  The results reach every rank by direct sends over the mesh, as the composite's strips do (composite.hip):
// rank j owns strip j of the image; one all-to-all brings the ranks' contributions to a strip -- zeros but for the one that
// finalised the pixel -- to its owner, the owner adds them up (integers: NaN and -0 survive), one all-gather returns the strips:
// 24 bytes per pixel cross each link once per phase, every link at once, where an all-reduce of the 7.4 MB (640 x 480) takes 14
// dependent ring steps.  KFX_SLAB_FINALISE=allreduce (or a transport without all_to_all / all_gather) keeps the all-reduce; same
// images.  `comm` and `stream` may be another communicator over the same ranks and another stream than the march's
// (kfx_slab_frame's pipelined frames): nothing here touches the march's planes.  h_open: a host-visible word that receives the
// number of pixels left without a final status (zero) once `stream` has passed.
int kfx::exact_tiled_finalise(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const ExactFinalBufs& fb, kfx_comm* comm,
                              kfx_stream stream, int* h_open)
{
    const int world = comm->world;
    const int w = (int)img->w, h = (int)img->h;
    hipStream_t s = (hipStream_t)stream;
    FirstError note;
    note(hip_status(hipMemsetAsync(fb.open, 0, sizeof(int), s), "kfx_slab_raycast_exact_tiled"));
    const bool direct = finalise_direct(comm);
    const unsigned S = direct ? (unsigned)fb.S : 0u;
    const int* final_planes = fb.contrib;
    if (direct) {
        const size_t words = 6 * fb.S;
        note(comm->all_to_all(comm, fb.contrib, fb.gathered, words * sizeof(int), stream));
        hipLaunchKernelGGL(k_strip_sum, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, fb.gathered, fb.mine, words, world);
        note(check_launch("kfx_slab_raycast_exact_tiled"));
        note(comm->all_gather(comm, fb.mine, fb.gathered, words * sizeof(int), stream));
        final_planes = fb.gathered;
    } else if (world > 1) {
        note(comm->all_reduce(comm, fb.contrib, 6 * (size_t)w * h, KFX_COMM_SUM_I32, stream));
    }
    hipLaunchKernelGGL(k_tiles_finish, pixel_grid(w, h), dim3(256), 0, s, render_images(depth, norm, img, img), final_planes, fb.open, S);
    note(check_launch("kfx_slab_raycast_exact_tiled"));
    if (h_open) note(hip_status(hipMemcpyAsync(h_open, fb.open, sizeof(int), hipMemcpyDeviceToHost, s), "kfx_slab_raycast_exact_tiled"));
    return note.status;
}

int kfx::exact_tiled(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, void* scratch, const kfx_volume* local,
                     const kfx_volume* color_local, const kfx_slab_layout* L, const float T_wc[12], const float K[4], float near, float far,
                     float trunc_dist, int subpix, int tiles, kfx_comm* comm, kfx_stream stream, int* h_open, int* steps_out)
{
    if (!scratch || !local || !L || !comm || !T_wc || !K) return set_error(KFX_E_NULL, "kfx_slab_raycast_exact_tiled: null argument");
    if (int e = check_layout(local, L, comm, "kfx_slab_raycast_exact_tiled")) return e;
    if (int e = check_render_images(depth, norm, img, img, "kfx_slab_raycast_exact_tiled")) return e;
    if ((uintptr_t)scratch & 15) return set_error(KFX_E_ALIGN, "kfx_slab_raycast_exact_tiled: scratch alignment");
    if (comm->world > 1 && !comm->exchange_v) return set_error(KFX_E_RANGE, "kfx_slab_raycast_exact_tiled: the transport has no exchange_v");
    if (color_local) {   // (every rank makes the same call with volumes of the same geometry: an argument error is every rank's)
        if (!local->ptr) return set_error(KFX_E_NULL, "kfx_slab_raycast_exact_tiled_color: null volume");
        if (int e = check_volume(color_local, 4, 1, VOLUME_MAX_DIM, "kfx_slab_raycast_exact_tiled_color")) return e;
        if (int e = check_color_slab(local, color_local, "kfx_slab_raycast_exact_tiled_color")) return e;
    }
    const int w = (int)img->w, h = (int)img->h;
    if (w == 0 || h == 0) return 0;
    TiledScratch t;
    tiled_layout(t, scratch, (size_t)w, (size_t)h, tiles, comm->world);
    // (a local failure of the march does not keep this rank out of the final exchange its peers enter)
    FirstError note;
    note(exact_tiled_march(t, t.own, local, L, T_wc, K, near, far, trunc_dist, subpix, w, h, comm, stream, steps_out, color_local));
    note(exact_tiled_finalise(depth, norm, img, t.own, comm, stream, h_open));
    if (h_open) return note.status;
    int n_open = 0;
    note(hip_status(hipMemcpyAsync(&n_open, t.own.open, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream), "kfx_slab_raycast_exact_tiled"));
    note(hip_status(hipStreamSynchronize((hipStream_t)stream), "kfx_slab_raycast_exact_tiled"));
    if (!note.status && n_open) note(set_error(KFX_E_RANGE, "kfx_slab_raycast_exact_tiled: rays without a final status after the hand-over"));
    return note.status;
}

extern "C" int kfx_slab_raycast_exact_tiled(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, void* scratch,
                                            const kfx_volume* local, const kfx_slab_layout* L, const float T_wc[12], const float K[4],
                                            float near, float far, float trunc_dist, int subpix, int tiles, kfx_comm* comm, kfx_stream stream,
                                            int* h_open, int* steps_out)
{
    return exact_tiled(depth, norm, img, scratch, local, nullptr, L, T_wc, K, near, far, trunc_dist, subpix, tiles, comm, stream, h_open, steps_out);
}

// the hand-over with this rank's colour slab (include/kfx_slab_color.h): the images of kfx_raycast_sdf_color on the whole volumes
extern "C" int kfx_slab_raycast_exact_tiled_color(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, void* scratch,
                                                  const kfx_volume* local, const kfx_volume* color_local, const kfx_slab_layout* L,
                                                  const float T_wc[12], const float K[4], float near, float far, float trunc_dist, int subpix,
                                                  int tiles, kfx_comm* comm, kfx_stream stream, int* h_open, int* steps_out)
{
    if (!color_local) return set_error(KFX_E_NULL, "kfx_slab_raycast_exact_tiled_color: null colour volume");
    return exact_tiled(depth, norm, img, scratch, local, color_local, L, T_wc, K, near, far, trunc_dist, subpix, tiles, comm, stream, h_open, steps_out);
}
