// mesh_clean.hip -- clean-up of an indexed mesh in device memory for gfx950 (include/kfx_mesh_clean.h): connected components of the
// face list, and the filter that drops the small ones and compacts the rest.  What every SaveMesh user does first with a KinectFusion
// mesh -- throw away the floaters that depth noise, unobserved cells and silhouettes leave around the surface -- without the mesh
// leaving HBM.  The host rules and the labelling rules (find / unite / root, with their invariants) are mesh_clean_host.h's.
//
// kfx_mesh_components_plan, in stream order after a memset of the header:
//   k_clean_validate   reads `faces` ALONE: an id >= V raises CLEAN_ERR_FACE_ID in the header.  Every later kernel of the plan tests
//                      the error word before it does anything, so no id from the caller is used as an address unchecked.
//   k_clean_init       parent[v] = v, cnt[v] = 0; the header's magic, V and T
//   k_clean_unite      one lane per face: unite(a, b), unite(b, c) on agent-scope atomics
//   k_clean_flatten    one lane per vertex: parent[v] = its root, the smallest id of its component
//   k_clean_count      one lane per face: cnt[root] += 1, aggregated per wave and, for the workgroup's first root, per workgroup
//   k_clean_roots      one lane per vertex: roots per block; the largest component (one 64-bit max per workgroup)
//   k_clean_scan       the blocks' first component ids and C
//   k_clean_seal       the stage, unless an error was raised
// kfx_mesh_components_emit: k_clean_rank (roots: their component id and its face count), k_clean_label (the others: their root's).
// kfx_mesh_filter_plan: k_filter_count (kept vertices and faces per block), k_clean_scan twice, k_filter_remap, k_clean_seal.
// kfx_mesh_filter_emit: k_filter_gather (rows of kept vertices as 32-bit words), k_filter_faces (kept faces through remap[]).
// Positions are handed out by scans alone (block_scan.h; partials -> base -> apply, as mesh.hip): no atomic orders anything, the
// atomics that remain are integer sums, maxima and links whose result does not depend on arrival order, so every output is a
// function of (V, faces) and the filter's parameters.
#include "host_args.h"
#include "mesh_clean_device.h"   // raise, block_sum, k_clean_validate, k_clean_scan: shared with mesh_simplify.hip

namespace kfx {

using u64 = unsigned long long;

// parent[] as the uniting and flattening launches reach it: every access an agent-scope relaxed atomic (the XCDs' L2s are private: a
// plain load could be served a stale line, a plain store could stay in one L2 -- the rules are correct under stale loads all the
// same, mesh_clean_host.h, but a link must be a device-wide compare-and-swap)
struct AgentParent {
    unsigned* parent;
    __device__ __forceinline__ unsigned load(unsigned i) const { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void store(unsigned i, unsigned v) const { __hip_atomic_store(parent + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ unsigned cas(unsigned i, unsigned expected, unsigned desired) const
    {
        __hip_atomic_compare_exchange_strong(parent + i, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;   // (the value found)
    }
};

__global__ __launch_bounds__(256) void k_clean_init(unsigned* __restrict__ parent, unsigned* __restrict__ cnt, const unsigned n_verts,
                                                    const unsigned n_faces, u64* __restrict__ hdr)
{
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v < n_verts) {
        parent[v] = v;
        cnt[v] = 0;
    }
    if (v == 0) {
        hdr[CLEAN_W_MAGIC] = CLEAN_MAGIC;
        hdr[CLEAN_W_VERTS] = n_verts;
        hdr[CLEAN_W_FACES] = n_faces;
    }
}

// Labelling (mesh_clean_host.h: clean_find / clean_unite, over AgentParent).
//   I1  parent[x] <= x, always.
//   I2  parent[x] is a vertex of x's true component, always.
//   I3  a root is linked only by an agent-scope compare-and-swap that expects the root itself.
// No lane waits for another lane, wave or workgroup: every loop descends strictly in vertex id and is capped at V steps besides; a
// walk beyond the cap raises CLEAN_ERR_WALK and leaves.
__global__ __launch_bounds__(256) void k_clean_unite(const unsigned* __restrict__ faces, const unsigned n_faces, const unsigned n_verts,
                                                     unsigned* parent, u64* hdr)
{
    if (hdr[CLEAN_W_ERROR]) return;
    const unsigned f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const unsigned a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    AgentParent m{parent};
    bool bad = false;
    if (a != b) clean_unite(m, a, b, n_verts, bad);
    if (b != c) clean_unite(m, b, c, n_verts, bad);
    if (bad) raise(hdr, CLEAN_ERR_WALK);
}

__global__ __launch_bounds__(256) void k_clean_flatten(unsigned* parent, const unsigned n_verts, u64* hdr)
{
    if (hdr[CLEAN_W_ERROR]) return;
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    AgentParent m{parent};
    bool bad = false;
    const unsigned r = clean_root(m, v, n_verts, bad);
    if (bad) raise(hdr, CLEAN_ERR_WALK);
    else if (r != v) m.store(v, r);
}

// cnt[root of the face's component] += 1.  The usual mesh is one big component: one atomic per face would serialise them all on one
// word.  So the lanes of a workgroup whose root is that of the workgroup's first face -- in that mesh, all of them -- are summed in
// LDS (a ballot per wave, one LDS add per wave) and leave as ONE add; the other lanes combine per wave, root by root (ballot of the
// lanes that share the first remaining lane's root), one add per distinct root.  No add's result is used; integer sums do not depend
// on order.
__global__ __launch_bounds__(256) void k_clean_count(const unsigned* __restrict__ faces, const unsigned n_faces, const unsigned* __restrict__ parent,
                                                     unsigned* cnt, const u64* __restrict__ hdr)
{
    if (hdr[CLEAN_W_ERROR]) return;
    __shared__ unsigned s_root, s_cnt;
    const unsigned f = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x == 0) {
        s_root = parent[faces[3 * (size_t)f]];   // (the grid has no empty workgroup)
        s_cnt = 0;
    }
    __syncthreads();
    const bool in = f < n_faces;
    const unsigned root = in ? parent[faces[3 * (size_t)f]] : 0u;
    const bool hot = in && root == s_root;
    const u64 hot_mask = __ballot(hot);
    if (lane == 0 && hot_mask) atomicAdd(&s_cnt, (unsigned)__popcll(hot_mask));
    bool rest = in && !hot;
    for (u64 mask = __ballot(rest); mask; mask = __ballot(rest)) {   // (wave-uniform; at most 64 turns: every turn retires its leader)
        const int leader = __ffsll((long long)mask) - 1;
        const unsigned r0 = __shfl(root, leader, 64);
        const bool same = rest && root == r0;
        const u64 same_mask = __ballot(same);
        if (lane == leader) __hip_atomic_fetch_add(cnt + r0, (unsigned)__popcll(same_mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rest = rest && !same;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) __hip_atomic_fetch_add(cnt + s_root, s_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// roots per block of 256 vertices, and the largest component: max of faces << 32 | ~root (ties go to the smaller root, which is the
// smaller component id: components are numbered in the order of their roots), one 64-bit max per workgroup
__global__ __launch_bounds__(256) void k_clean_roots(const unsigned* __restrict__ parent, const unsigned* __restrict__ cnt, const unsigned n_verts,
                                                     unsigned* __restrict__ rpart, u64* hdr)
{
    if (hdr[CLEAN_W_ERROR]) return;
    __shared__ u64 s_best[4];
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    const bool root = v < n_verts && parent[v] == v;
    u64 key = root ? clean_best_key(v, cnt[v]) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = key;
    const unsigned total = block_sum(root ? 1u : 0u);   // (its barriers order s_best too)
    if (threadIdx.x == 0) {
        rpart[blockIdx.x] = total;
        u64 best = s_best[0];
        for (int i = 1; i < 4; ++i) best = s_best[i] > best ? s_best[i] : best;
        if (best) __hip_atomic_fetch_max(hdr + CLEAN_W_BEST, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the stage a plan has reached and, of a filter plan, its parameters -- unless an error was raised
__global__ void k_clean_seal(u64* hdr, const u64 stage, const u64 min_faces, const u64 largest)
{
    if (hdr[CLEAN_W_ERROR]) return;
    hdr[CLEAN_W_STAGE] = stage;
    hdr[CLEAN_W_MIN_FACES] = min_faces;
    hdr[CLEAN_W_LARGEST] = largest;
}

// roots: their component id -- the roots before them -- and its face count
__global__ __launch_bounds__(256) void k_clean_rank(const unsigned* __restrict__ parent, const unsigned* __restrict__ cnt, const unsigned n_verts,
                                                    const unsigned* __restrict__ rbase, unsigned* __restrict__ vertex_component,
                                                    unsigned* __restrict__ component_faces)
{
    __shared__ unsigned lds[4];
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    const bool root = v < n_verts && parent[v] == v;
    unsigned total;
    const unsigned rank = rbase[blockIdx.x] + block_exclusive_scan<unsigned, 4>(root ? 1u : 0u, lds, &total);
    if (root) {
        vertex_component[v] = rank;
        component_faces[rank] = cnt[v];
    }
}
// the others: their root's (written by the launch before; this one writes no root's)
__global__ __launch_bounds__(256) void k_clean_label(const unsigned* __restrict__ parent, const unsigned n_verts, unsigned* vertex_component)
{
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    const unsigned r = parent[v];
    if (r != v) vertex_component[v] = vertex_component[r];
}

struct CleanFilter {
    u64 min_faces;
    int largest;
};
// whether the filter keeps the component of root r
__device__ __forceinline__ bool keeps(const CleanFilter& q, const unsigned* __restrict__ cnt, const u64* __restrict__ hdr, unsigned r)
{
    return clean_keeps(r, cnt[r], q.min_faces, q.largest, hdr[CLEAN_W_BEST]);
}

// kept vertices per block of 256 vertices (workgroups [0, vblk)) and kept faces per block of 256 faces (the workgroups after them)
__global__ __launch_bounds__(256) void k_filter_count(const unsigned* __restrict__ faces, const unsigned n_faces, const unsigned n_verts,
                                                      const unsigned* __restrict__ parent, const unsigned* __restrict__ cnt,
                                                      const u64* __restrict__ hdr, const CleanFilter q, const unsigned vblk,
                                                      unsigned* __restrict__ vpart, unsigned* __restrict__ fpart)
{
    bool keep;
    if (blockIdx.x < vblk) {
        const unsigned v = blockIdx.x * 256 + threadIdx.x;
        keep = v < n_verts && keeps(q, cnt, hdr, parent[v]);
    } else {
        const unsigned f = (blockIdx.x - vblk) * 256 + threadIdx.x;
        keep = false;
        if (f < n_faces) {   // (the ids were checked by the plan; a caller who has changed `faces` since gets no address out of them)
            const unsigned a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
            keep = a < n_verts && b < n_verts && c < n_verts && keeps(q, cnt, hdr, parent[a]);
        }
    }
    const unsigned total = block_sum(keep ? 1u : 0u);
    if (threadIdx.x == 0) (blockIdx.x < vblk ? vpart[blockIdx.x] : fpart[blockIdx.x - vblk]) = total;
}

// every vertex's id after the filter: the kept vertices before it
__global__ __launch_bounds__(256) void k_filter_remap(const unsigned* __restrict__ parent, const unsigned* __restrict__ cnt, const unsigned n_verts,
                                                      const u64* __restrict__ hdr, const CleanFilter q, const unsigned* __restrict__ vbase,
                                                      unsigned* __restrict__ remap)
{
    __shared__ unsigned lds[4];
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    const bool keep = v < n_verts && keeps(q, cnt, hdr, parent[v]);
    unsigned total;
    const unsigned at = vbase[blockIdx.x] + block_exclusive_scan<unsigned, 4>(keep ? 1u : 0u, lds, &total);
    if (v < n_verts) remap[v] = keep ? at : CLEAN_DROPPED;
}

// The rows of the kept vertices, copied as 32-bit words (NaN payloads and all).  C16: both colour arrays are 16-byte aligned and a
// colour row moves as one 16-byte lane; positions and normals are 12-byte rows on 4-byte alignment and move as three words.
template <bool C16>
__global__ __launch_bounds__(256) void k_filter_gather(const unsigned* __restrict__ remap, const unsigned n_verts, const unsigned* __restrict__ verts,
                                                       const unsigned* __restrict__ norms, const unsigned* __restrict__ colors,
                                                       unsigned* __restrict__ verts_out, unsigned* __restrict__ norms_out, unsigned* __restrict__ colors_out)
{
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    const unsigned at = remap[v];
    if (at == CLEAN_DROPPED) return;
    const size_t i = v, o = at;
#pragma unroll
    for (int k = 0; k < 3; ++k) verts_out[3 * o + k] = verts[3 * i + k];
    if (norms) {
#pragma unroll
        for (int k = 0; k < 3; ++k) norms_out[3 * o + k] = norms[3 * i + k];
    }
    if (colors) {
        if (C16) {
            ((uint4*)colors_out)[o] = ((const uint4*)colors)[i];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) colors_out[4 * o + k] = colors[4 * i + k];
        }
    }
}

// the kept faces, in their order, their ids through remap[] (a face is kept with its component, so with all its vertices)
__global__ __launch_bounds__(256) void k_filter_faces(const unsigned* __restrict__ faces, const unsigned n_faces, const unsigned n_verts,
                                                      const unsigned* __restrict__ remap, const unsigned* __restrict__ fbase,
                                                      unsigned* __restrict__ faces_out)
{
    __shared__ unsigned lds[4];
    const unsigned f = blockIdx.x * 256 + threadIdx.x;
    unsigned id[3] = {CLEAN_DROPPED, CLEAN_DROPPED, CLEAN_DROPPED};
    if (f < n_faces) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned v = faces[3 * (size_t)f + k];
            id[k] = v < n_verts ? remap[v] : CLEAN_DROPPED;   // (k_filter_count's rule)
        }
    }
    const bool keep = id[0] != CLEAN_DROPPED && id[1] != CLEAN_DROPPED && id[2] != CLEAN_DROPPED;
    unsigned total;
    const size_t at = fbase[blockIdx.x] + block_exclusive_scan<unsigned, 4>(keep ? 1u : 0u, lds, &total);
    if (keep) {
#pragma unroll
        for (int k = 0; k < 3; ++k) faces_out[3 * at + k] = id[k];
    }
}

// ---- host side ----

struct CleanCall {
    CleanScratch s;
    u64* hdr;
    unsigned *parent, *cnt, *remap, *rpart, *rbase, *vpart, *vbase, *fpart, *fbase;
};

// the counts and the scratch of every call, before any HIP call
static int clean_call(CleanCall& c, const char* what, u64 n_verts, u64 n_faces, const void* scratch, size_t scratch_bytes)
{
    if (int e = refuse(clean_check_counts(n_verts, n_faces), what)) return e;
    if (int e = refuse(clean_check_scratch(n_verts, n_faces, scratch, scratch_bytes), what)) return e;
    c.s = clean_scratch(n_verts, n_faces);
    unsigned char* const at = (unsigned char*)scratch;
    c.hdr = (u64*)(at + c.s.hdr);
    c.parent = (unsigned*)(at + c.s.parent); c.cnt = (unsigned*)(at + c.s.cnt); c.remap = (unsigned*)(at + c.s.remap);
    c.rpart = (unsigned*)(at + c.s.rpart); c.rbase = (unsigned*)(at + c.s.rbase);
    c.vpart = (unsigned*)(at + c.s.vpart); c.vbase = (unsigned*)(at + c.s.vbase);
    c.fpart = (unsigned*)(at + c.s.fpart); c.fbase = (unsigned*)(at + c.s.fbase);
    return 0;
}

// the header, once the stream's earlier work is done
static int read_clean_header(u64* host, const u64* hdr, hipStream_t st)
{
    hipError_t e = hipMemcpyAsync(host, hdr, CLEAN_WORDS * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : set_error((int)e, hipGetErrorString(e));
}

// "The scratch is this mesh's plan": magic, V, T, and a stage of at least `stage`
static int check_clean_scratch(u64* host, const CleanCall& c, u64 n_verts, u64 n_faces, u64 stage, const char* what, hipStream_t st)
{
    if (int e = read_clean_header(host, c.hdr, st)) return e;
    if (host[CLEAN_W_MAGIC] != CLEAN_MAGIC || host[CLEAN_W_VERTS] != n_verts || host[CLEAN_W_FACES] != n_faces || host[CLEAN_W_STAGE] < stage ||
        host[CLEAN_W_STAGE] > CLEAN_STAGE_FILTERED || host[CLEAN_W_ERROR])
        return fail_rule(what, KFX_E_RANGE, "the scratch is not this mesh's plan");
    return 0;
}

static int clean_device_error(u64 bits, const char* what)
{
    if (bits & CLEAN_ERR_FACE_ID) return fail_rule(what, KFX_E_RANGE, "a face id >= n_verts");
    return fail_rule(what, KFX_E_RANGE, "a labelling walk exceeded its cap");
}

static unsigned blocks_of(u64 n) { return (unsigned)((n + CLEAN_BLOCK - 1) / CLEAN_BLOCK); }

} // namespace kfx

using namespace kfx;

extern "C" size_t kfx_mesh_components_scratch_bytes(unsigned long long n_verts, unsigned long long n_faces)
{
    if (clean_check_counts(n_verts, n_faces).code) return 0;
    return clean_scratch(n_verts, n_faces).bytes;
}

extern "C" int kfx_mesh_components_plan(const unsigned* faces, unsigned long long n_faces, unsigned long long n_verts, void* scratch,
                                        size_t scratch_bytes, unsigned long long counts_out[2], kfx_stream stream)
{
    const char* const what = "kfx_mesh_components_plan";
    if (!counts_out) return fail_rule(what, KFX_E_NULL, "null counts_out");
    CleanCall c;
    if (int e = clean_call(c, what, n_verts, n_faces, scratch, scratch_bytes)) return e;
    if (n_faces && !faces) return fail_rule(what, KFX_E_NULL, "null faces");
    if ((uintptr_t)faces & 3) return fail_rule(what, KFX_E_ALIGN, "faces not aligned to 4 bytes");
    counts_out[0] = counts_out[1] = 0;
    if (n_faces == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    const unsigned V = (unsigned)n_verts, T = (unsigned)n_faces;
    if (hipError_t e = hipMemsetAsync(c.hdr, 0, 256, st); e != hipSuccess) return set_error((int)e, hipGetErrorString(e));
    hipLaunchKernelGGL(k_clean_validate, dim3(blocks_of(3 * n_faces)), dim3(256), 0, st, faces, 3 * n_faces, V, c.hdr);
    hipLaunchKernelGGL(k_clean_init, dim3(blocks_of(n_verts)), dim3(256), 0, st, c.parent, c.cnt, V, T, c.hdr);
    hipLaunchKernelGGL(k_clean_unite, dim3(blocks_of(n_faces)), dim3(256), 0, st, faces, T, V, c.parent, c.hdr);
    hipLaunchKernelGGL(k_clean_flatten, dim3(blocks_of(n_verts)), dim3(256), 0, st, c.parent, V, c.hdr);
    hipLaunchKernelGGL(k_clean_count, dim3(blocks_of(n_faces)), dim3(256), 0, st, faces, T, c.parent, c.cnt, c.hdr);
    hipLaunchKernelGGL(k_clean_roots, dim3(blocks_of(n_verts)), dim3(256), 0, st, c.parent, c.cnt, V, c.rpart, c.hdr);
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(CLEAN_SCAN_THREADS), 0, st, c.rpart, (unsigned)c.s.vblk, c.rbase, c.hdr, (int)CLEAN_W_COMPONENTS);
    hipLaunchKernelGGL(k_clean_seal, dim3(1), dim3(1), 0, st, c.hdr, (u64)CLEAN_STAGE_LABELLED, 0ull, 0ull);
    if (int e = check_launch(what)) return e;
    u64 host[CLEAN_WORDS];
    if (int e = read_clean_header(host, c.hdr, st)) return e;
    if (host[CLEAN_W_ERROR]) return clean_device_error(host[CLEAN_W_ERROR], what);
    counts_out[0] = host[CLEAN_W_COMPONENTS];
    counts_out[1] = host[CLEAN_W_BEST] >> 32;
    return 0;
}

extern "C" int kfx_mesh_components_emit(const void* scratch, size_t scratch_bytes, unsigned long long n_verts, unsigned long long n_faces,
                                        const unsigned long long counts[2], unsigned* vertex_component, unsigned* component_faces,
                                        kfx_stream stream)
{
    const char* const what = "kfx_mesh_components_emit";
    CleanCall c;
    if (int e = clean_call(c, what, n_verts, n_faces, scratch, scratch_bytes)) return e;
    if (n_faces == 0) return 0;
    if (int e = refuse(clean_check_planned(n_verts, n_faces, counts, false), what)) return e;
    if (int e = refuse(clean_check_array(vertex_component, false), what)) return e;
    if (int e = refuse(clean_check_array(component_faces, false), what)) return e;
    if (clean_ranges_overlap(vertex_component, 4 * n_verts, component_faces, 4 * counts[0]) ||
        clean_ranges_overlap(vertex_component, 4 * n_verts, scratch, scratch_bytes) || clean_ranges_overlap(component_faces, 4 * counts[0], scratch, scratch_bytes))
        return fail_rule(what, KFX_E_RANGE, "the outputs overlap each other or the scratch");
    const hipStream_t st = (hipStream_t)stream;
    u64 host[CLEAN_WORDS];
    if (int e = check_clean_scratch(host, c, n_verts, n_faces, CLEAN_STAGE_LABELLED, what, st)) return e;
    if (host[CLEAN_W_COMPONENTS] != counts[0] || host[CLEAN_W_BEST] >> 32 != counts[1]) return fail_rule(what, KFX_E_RANGE, "counts are not the plan's");
    const unsigned V = (unsigned)n_verts;
    hipLaunchKernelGGL(k_clean_rank, dim3(blocks_of(n_verts)), dim3(256), 0, st, c.parent, c.cnt, V, c.rbase, vertex_component, component_faces);
    hipLaunchKernelGGL(k_clean_label, dim3(blocks_of(n_verts)), dim3(256), 0, st, c.parent, V, vertex_component);
    return check_launch(what);
}

extern "C" int kfx_mesh_filter_plan(void* scratch, size_t scratch_bytes, unsigned long long n_verts, unsigned long long n_faces,
                                    const unsigned* faces, unsigned long long min_faces, int largest, unsigned long long out[2], kfx_stream stream)
{
    const char* const what = "kfx_mesh_filter_plan";
    if (!out) return fail_rule(what, KFX_E_NULL, "null out");
    CleanCall c;
    if (int e = clean_call(c, what, n_verts, n_faces, scratch, scratch_bytes)) return e;
    if (n_faces && !faces) return fail_rule(what, KFX_E_NULL, "null faces");
    if ((uintptr_t)faces & 3) return fail_rule(what, KFX_E_ALIGN, "faces not aligned to 4 bytes");
    out[0] = out[1] = 0;
    if (n_faces == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    u64 host[CLEAN_WORDS];
    if (int e = check_clean_scratch(host, c, n_verts, n_faces, CLEAN_STAGE_LABELLED, what, st)) return e;
    const unsigned V = (unsigned)n_verts, T = (unsigned)n_faces, vblk = (unsigned)c.s.vblk, fblk = (unsigned)c.s.fblk;
    const CleanFilter q{min_faces, largest != 0};
    hipLaunchKernelGGL(k_filter_count, dim3(vblk + fblk), dim3(256), 0, st, faces, T, V, c.parent, c.cnt, c.hdr, q, vblk, c.vpart, c.fpart);
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(CLEAN_SCAN_THREADS), 0, st, c.vpart, vblk, c.vbase, c.hdr, (int)CLEAN_W_KEPT_VERTS);
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(CLEAN_SCAN_THREADS), 0, st, c.fpart, fblk, c.fbase, c.hdr, (int)CLEAN_W_KEPT_FACES);
    hipLaunchKernelGGL(k_filter_remap, dim3(vblk), dim3(256), 0, st, c.parent, c.cnt, V, c.hdr, q, c.vbase, c.remap);
    hipLaunchKernelGGL(k_clean_seal, dim3(1), dim3(1), 0, st, c.hdr, (u64)CLEAN_STAGE_FILTERED, (u64)min_faces, (u64)(largest != 0));
    if (int e = check_launch(what)) return e;
    if (int e = read_clean_header(host, c.hdr, st)) return e;
    out[0] = host[CLEAN_W_KEPT_VERTS];
    out[1] = host[CLEAN_W_KEPT_FACES];
    return 0;
}

extern "C" int kfx_mesh_filter_emit(const void* scratch, size_t scratch_bytes, unsigned long long n_verts, unsigned long long n_faces,
                                    const unsigned long long kept[2], const float* verts, const float* norms, const float* colors,
                                    const unsigned* faces, float* verts_out, float* norms_out, float* colors_out, unsigned* faces_out,
                                    kfx_stream stream)
{
    const char* const what = "kfx_mesh_filter_emit";
    CleanCall c;
    if (int e = clean_call(c, what, n_verts, n_faces, scratch, scratch_bytes)) return e;
    if (n_faces == 0) return 0;
    if (int e = refuse(clean_check_planned(n_verts, n_faces, kept, true), what)) return e;
    const void* const in[4] = {verts, norms, colors, faces};
    const void* const outs[4] = {verts_out, norms_out, colors_out, faces_out};
    if (int e = refuse(clean_check_filter_arrays(n_verts, n_faces, kept, in, outs, scratch, scratch_bytes), what)) return e;
    const hipStream_t st = (hipStream_t)stream;
    u64 host[CLEAN_WORDS];
    if (int e = check_clean_scratch(host, c, n_verts, n_faces, CLEAN_STAGE_FILTERED, what, st)) return e;
    if (host[CLEAN_W_KEPT_VERTS] != kept[0] || host[CLEAN_W_KEPT_FACES] != kept[1]) return fail_rule(what, KFX_E_RANGE, "kept counts are not the filter plan's");
    if (kept[0] == 0) return 0;
    const unsigned V = (unsigned)n_verts, T = (unsigned)n_faces;
    const unsigned* const n_in = norms && norms_out ? (const unsigned*)norms : nullptr;
    const unsigned* const c_in = colors && colors_out ? (const unsigned*)colors : nullptr;
    const bool c16 = c_in && !(((uintptr_t)colors | (uintptr_t)colors_out) & 15);
    auto gather = c16 ? k_filter_gather<true> : k_filter_gather<false>;
    hipLaunchKernelGGL(gather, dim3(blocks_of(n_verts)), dim3(256), 0, st, c.remap, V, (const unsigned*)verts, n_in, c_in, (unsigned*)verts_out,
                       (unsigned*)norms_out, (unsigned*)colors_out);
    if (kept[1])
        hipLaunchKernelGGL(k_filter_faces, dim3(blocks_of(n_faces)), dim3(256), 0, st, faces, T, V, c.remap, c.fbase, faces_out);
    return check_launch(what);
}
