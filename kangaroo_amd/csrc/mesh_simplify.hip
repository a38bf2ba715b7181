// mesh_simplify.hip -- level of detail for an indexed mesh in device memory for gfx950 (include/kfx_mesh_simplify.h): vertex clustering
// on a world-anchored grid.  The last stage of the mesh pipeline and the one whose output is smaller than its input: a volume fused at
// 2 mm can hand out a 1 cm mesh without the fine one leaving HBM.  The host rules, the key rules and the table rules (insert / find,
// with what makes them safe under any interleaving) are mesh_simplify_host.h's.
//
// kfx_mesh_simplify_plan, in stream order after a memset of the header:
//   k_clean_validate      (mesh_clean_device.h) reads `faces` ALONE: an id >= V raises the face-id bit in the header.  Every later kernel of
//                         the plan tests the error word before it does anything, so no id from the caller is used as an address unchecked.
//   k_simplify_init       both tables free, used[] = 0; the header's magic, V and T
//   k_simplify_vinsert    one lane per vertex: its cell's slot is claimed by a compare-and-swap or lowered by a 64-bit minimum of
//                         d2 bits << 32 | id, on agent-scope atomics
//   k_simplify_vfind      one lane per vertex, read-only on the table: rep[v] = the vertex its cell's slot names
//   k_simplify_finsert    one lane per face with three distinct clusters: the slot of its sorted triple is claimed or lowered to
//                         the smaller face id
//   k_simplify_fmark      one lane per face, read-only on the table: kept iff the slot of its triple names it; a kept face marks its
//                         three representatives as used; kept faces per block
//   k_simplify_vcount     written representatives per block
//   k_clean_scan          (mesh_clean_device.h) twice: the blocks' first new ids, V' and T'
//   k_simplify_remap      every written representative's new id
//   k_simplify_seal       the stage, unless an error was raised
// kfx_mesh_simplify_emit: k_simplify_gather (rows of the written representatives as 32-bit words; vertex_cluster[]),
// k_simplify_faces (kept faces through rep[] and remap[]).
// Positions are handed out by scans alone (block_scan.h): no atomic orders anything.  The atomics that remain are claims of free
// slots and integer minima; which slot a key ends in depends on arrival, what the slot holds at the end does not: the minimum over
// its key's entries.  So every output is a function of the inputs and the grid.  No lane waits for another: a probe either finishes
// or moves to the next slot, and is capped at the table's capacity; beyond the cap it raises SIMPLIFY_ERR_PROBE and leaves.
#include "host_args.h"
#include "mesh_clean_device.h"   // raise, block_sum, k_clean_validate, k_clean_scan: shared with mesh_clean.hip
#include "mesh_simplify_host.h"

namespace kfx {

using u64 = unsigned long long;

// a table's slots as the inserting launches reach them: every access an agent-scope relaxed atomic (the XCDs' L2s are private: a
// plain load could be served a stale line -- the rules are correct under stale loads all the same, mesh_simplify_host.h, but a claim
// and a minimum must be device-wide)
template <typename WORD>
struct AgentSlots {
    WORD* slots;
    __device__ __forceinline__ WORD load(u64 s) const { return __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ WORD cas(u64 s, WORD expected, WORD desired) const
    {
        __hip_atomic_compare_exchange_strong(slots + s, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;   // (the value found)
    }
    __device__ __forceinline__ void min(u64 s, WORD word) const { __hip_atomic_fetch_min(slots + s, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// ... and as the launches after them do: the table no longer changes
template <typename WORD>
struct PlainSlots {
    const WORD* slots;
    __device__ __forceinline__ WORD load(u64 s) const { return slots[s]; }
};

// a grid-stride loop: the tables have up to 2^33 slots
__global__ __launch_bounds__(256) void k_simplify_init(u64* __restrict__ vtab, const u64 vcap, unsigned* __restrict__ ftab, const u64 fcap,
                                                       unsigned* __restrict__ used, const unsigned n_verts, const unsigned n_faces, u64* __restrict__ hdr)
{
    const u64 first = (u64)blockIdx.x * 256 + threadIdx.x, step = (u64)gridDim.x * 256;
    for (u64 i = first; i < vcap; i += step) vtab[i] = SIMPLIFY_VEMPTY;
    for (u64 i = first; i < fcap; i += step) ftab[i] = SIMPLIFY_FEMPTY;
    for (u64 i = first; i < n_verts; i += step) used[i] = 0;
    if (first == 0) {
        hdr[SIMPLIFY_W_MAGIC] = SIMPLIFY_MAGIC;
        hdr[SIMPLIFY_W_VERTS] = n_verts;
        hdr[SIMPLIFY_W_FACES] = n_faces;
    }
}

__global__ __launch_bounds__(256) void k_simplify_vinsert(const float* __restrict__ verts, const unsigned n_verts, const SimplifyGrid g, u64* vtab,
                                                          const u64 vmask, u64* hdr)
{
    if (hdr[SIMPLIFY_W_ERROR]) return;
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    const SimplifyVertex me = simplify_vertex(verts + 3 * (size_t)v, g, v);
    AgentSlots<u64> m{vtab};
    if (!simplify_insert<u64>(m, vmask, me.key, simplify_vertex_word(me, v), SimplifyVertexKeyOf{verts, g})) raise(hdr, SIMPLIFY_ERR_PROBE);
}

__global__ __launch_bounds__(256) void k_simplify_vfind(const float* __restrict__ verts, const unsigned n_verts, const SimplifyGrid g,
                                                        const u64* __restrict__ vtab, const u64 vmask, unsigned* __restrict__ rep, u64* hdr)
{
    if (hdr[SIMPLIFY_W_ERROR]) return;
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    const SimplifyVertex me = simplify_vertex(verts + 3 * (size_t)v, g, v);
    const u64 word = simplify_find<u64>(PlainSlots<u64>{vtab}, vmask, me.key, SimplifyVertexKeyOf{verts, g});
    if (word == SIMPLIFY_VEMPTY) {   // (its own insert put the key there)
        raise(hdr, SIMPLIFY_ERR_PROBE);
        rep[v] = v;
    } else
        rep[v] = (unsigned)word;
}

__global__ __launch_bounds__(256) void k_simplify_finsert(const unsigned* __restrict__ faces, const unsigned n_faces, const unsigned* __restrict__ rep,
                                                          unsigned* ftab, const u64 fmask, u64* hdr)
{
    if (hdr[SIMPLIFY_W_ERROR]) return;
    const unsigned f = blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const SimplifyFaceKeyOf key_of{faces, rep};
    const SimplifyTriple me = key_of(f);
    if (me.degenerate()) return;
    AgentSlots<unsigned> m{ftab};
    if (!simplify_insert<unsigned>(m, fmask, me, f, key_of)) raise(hdr, SIMPLIFY_ERR_PROBE);
}

// kept: three distinct clusters, and the smallest face id of its triple.  used[] takes plain stores of 1 from whoever gets there.
__global__ __launch_bounds__(256) void k_simplify_fmark(const unsigned* __restrict__ faces, const unsigned n_faces, const unsigned* __restrict__ rep,
                                                        const unsigned* __restrict__ ftab, const u64 fmask, unsigned* __restrict__ fkeep,
                                                        unsigned* used, unsigned* __restrict__ fpart, const u64* __restrict__ hdr)
{
    if (hdr[SIMPLIFY_W_ERROR]) return;
    const unsigned f = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (f < n_faces) {
        const SimplifyFaceKeyOf key_of{faces, rep};
        const SimplifyTriple me = key_of(f);
        keep = !me.degenerate() && simplify_find<unsigned>(PlainSlots<unsigned>{ftab}, fmask, me, key_of) == f;
        fkeep[f] = keep ? 1u : 0u;
        if (keep) used[me.a] = used[me.b] = used[me.c] = 1u;
    }
    const unsigned total = block_sum(keep ? 1u : 0u);
    if (threadIdx.x == 0) fpart[blockIdx.x] = total;
}

// whether v's row is written: it is a representative and a kept face refers to it
__device__ __forceinline__ bool simplify_written(const unsigned* __restrict__ rep, const unsigned* __restrict__ used, unsigned v) { return rep[v] == v && used[v]; }

__global__ __launch_bounds__(256) void k_simplify_vcount(const unsigned* __restrict__ rep, const unsigned* __restrict__ used, const unsigned n_verts,
                                                         unsigned* __restrict__ vpart, const u64* __restrict__ hdr)
{
    if (hdr[SIMPLIFY_W_ERROR]) return;
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    const unsigned total = block_sum(v < n_verts && simplify_written(rep, used, v) ? 1u : 0u);
    if (threadIdx.x == 0) vpart[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_simplify_remap(const unsigned* __restrict__ rep, const unsigned* __restrict__ used, const unsigned n_verts,
                                                        const unsigned* __restrict__ vbase, unsigned* __restrict__ remap, const u64* __restrict__ hdr)
{
    if (hdr[SIMPLIFY_W_ERROR]) return;
    __shared__ unsigned lds[4];
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    const bool keep = v < n_verts && simplify_written(rep, used, v);
    unsigned total;
    const unsigned at = vbase[blockIdx.x] + block_exclusive_scan<unsigned, 4>(keep ? 1u : 0u, lds, &total);
    if (v < n_verts) remap[v] = keep ? at : CLEAN_DROPPED;
}

__global__ void k_simplify_seal(u64* hdr, const u64 stage)
{
    if (hdr[SIMPLIFY_W_ERROR]) return;
    hdr[SIMPLIFY_W_STAGE] = stage;
}

// The rows of the written representatives, copied as 32-bit words (NaN payloads and all), and every vertex's new id.  C16: both colour
// arrays are 16-byte aligned and a colour row moves as one 16-byte lane.
template <bool C16>
__global__ __launch_bounds__(256) void k_simplify_gather(const unsigned* __restrict__ rep, const unsigned* __restrict__ remap, const unsigned n_verts,
                                                         const unsigned* __restrict__ verts, const unsigned* __restrict__ norms,
                                                         const unsigned* __restrict__ colors, unsigned* __restrict__ verts_out,
                                                         unsigned* __restrict__ norms_out, unsigned* __restrict__ colors_out,
                                                         unsigned* __restrict__ vertex_cluster)
{
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    const unsigned at = remap[v];
    if (vertex_cluster) {
        const unsigned r = rep[v];
        vertex_cluster[v] = r < n_verts ? remap[r] : CLEAN_DROPPED;
    }
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

// the kept faces, in their order and winding, their ids through rep[] and remap[] (a kept face's representatives are all written)
__global__ __launch_bounds__(256) void k_simplify_faces(const unsigned* __restrict__ faces, const unsigned n_faces, const unsigned n_verts,
                                                        const unsigned* __restrict__ fkeep, const unsigned* __restrict__ rep,
                                                        const unsigned* __restrict__ remap, const unsigned* __restrict__ fbase,
                                                        unsigned* __restrict__ faces_out)
{
    __shared__ unsigned lds[4];
    const unsigned f = blockIdx.x * 256 + threadIdx.x;
    unsigned id[3] = {CLEAN_DROPPED, CLEAN_DROPPED, CLEAN_DROPPED};
    if (f < n_faces && fkeep[f]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // (the ids were checked by the plan; a caller who has changed `faces` since gets no address out of them)
            const unsigned v = faces[3 * (size_t)f + k];
            const unsigned r = v < n_verts ? rep[v] : CLEAN_DROPPED;
            id[k] = r < n_verts ? remap[r] : CLEAN_DROPPED;
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

struct SimplifyCall {
    SimplifyScratch s;
    u64 *hdr, *vtab;
    unsigned *ftab, *rep, *used, *remap, *fkeep, *vpart, *vbase, *fpart, *fbase;
};

// the counts and the scratch of every call, before any HIP call
static int simplify_call(SimplifyCall& c, const char* what, u64 n_verts, u64 n_faces, const void* scratch, size_t scratch_bytes)
{
    if (int e = refuse(clean_check_counts(n_verts, n_faces), what)) return e;
    if (int e = refuse(simplify_check_scratch(n_verts, n_faces, scratch, scratch_bytes), what)) return e;
    c.s = simplify_scratch(n_verts, n_faces);
    unsigned char* const at = (unsigned char*)scratch;
    c.hdr = (u64*)(at + c.s.hdr); c.vtab = (u64*)(at + c.s.vtab);
    c.ftab = (unsigned*)(at + c.s.ftab); c.rep = (unsigned*)(at + c.s.rep); c.used = (unsigned*)(at + c.s.used);
    c.remap = (unsigned*)(at + c.s.remap); c.fkeep = (unsigned*)(at + c.s.fkeep);
    c.vpart = (unsigned*)(at + c.s.vpart); c.vbase = (unsigned*)(at + c.s.vbase);
    c.fpart = (unsigned*)(at + c.s.fpart); c.fbase = (unsigned*)(at + c.s.fbase);
    return 0;
}

// the header, once the stream's earlier work is done
static int read_simplify_header(u64* host, const u64* hdr, hipStream_t st)
{
    hipError_t e = hipMemcpyAsync(host, hdr, SIMPLIFY_WORDS * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : set_error((int)e, hipGetErrorString(e));
}

static unsigned simplify_blocks_of(u64 n) { return (unsigned)((n + CLEAN_BLOCK - 1) / CLEAN_BLOCK); }

} // namespace kfx

using namespace kfx;

extern "C" size_t kfx_mesh_simplify_scratch_bytes(unsigned long long n_verts, unsigned long long n_faces)
{
    if (clean_check_counts(n_verts, n_faces).code) return 0;
    return simplify_scratch(n_verts, n_faces).bytes;
}

extern "C" int kfx_mesh_simplify_plan(const float* verts, const unsigned* faces, unsigned long long n_faces, unsigned long long n_verts,
                                      const float origin[3], float cell, void* scratch, size_t scratch_bytes, unsigned long long out[2],
                                      kfx_stream stream)
{
    const char* const what = "kfx_mesh_simplify_plan";
    if (!out) return fail_rule(what, KFX_E_NULL, "null out");
    SimplifyCall c;
    if (int e = simplify_call(c, what, n_verts, n_faces, scratch, scratch_bytes)) return e;
    if (n_faces && !faces) return fail_rule(what, KFX_E_NULL, "null faces");
    if (n_faces && !verts) return fail_rule(what, KFX_E_NULL, "null verts");
    if (((uintptr_t)faces | (uintptr_t)verts) & 3) return fail_rule(what, KFX_E_ALIGN, "verts or faces not aligned to 4 bytes");
    SimplifyGrid g;
    if (int e = refuse(simplify_check_grid(origin, cell, &g), what)) return e;
    if (clean_ranges_overlap(scratch, scratch_bytes, verts, 12 * n_verts) || clean_ranges_overlap(scratch, scratch_bytes, faces, 12 * n_faces))
        return fail_rule(what, KFX_E_RANGE, "the scratch overlaps an input");
    out[0] = out[1] = 0;
    if (n_faces == 0) return 0;
    const hipStream_t st = (hipStream_t)stream;
    const unsigned V = (unsigned)n_verts, T = (unsigned)n_faces, vblk = (unsigned)c.s.vblk, fblk = (unsigned)c.s.fblk;
    const u64 vmask = c.s.vcap - 1, fmask = c.s.fcap - 1;
    const u64 init_items = c.s.vcap > c.s.fcap ? c.s.vcap : c.s.fcap;
    const unsigned init_blocks = (unsigned)(init_items / 256 < 65536 ? init_items / 256 : 65536);
    if (hipError_t e = hipMemsetAsync(c.hdr, 0, 256, st); e != hipSuccess) return set_error((int)e, hipGetErrorString(e));
    hipLaunchKernelGGL(k_clean_validate, dim3(simplify_blocks_of(3 * n_faces)), dim3(256), 0, st, faces, 3 * n_faces, V, c.hdr);
    hipLaunchKernelGGL(k_simplify_init, dim3(init_blocks ? init_blocks : 1), dim3(256), 0, st, c.vtab, c.s.vcap, c.ftab, c.s.fcap, c.used, V, T, c.hdr);
    hipLaunchKernelGGL(k_simplify_vinsert, dim3(vblk), dim3(256), 0, st, verts, V, g, c.vtab, vmask, c.hdr);
    hipLaunchKernelGGL(k_simplify_vfind, dim3(vblk), dim3(256), 0, st, verts, V, g, c.vtab, vmask, c.rep, c.hdr);
    hipLaunchKernelGGL(k_simplify_finsert, dim3(fblk), dim3(256), 0, st, faces, T, c.rep, c.ftab, fmask, c.hdr);
    hipLaunchKernelGGL(k_simplify_fmark, dim3(fblk), dim3(256), 0, st, faces, T, c.rep, c.ftab, fmask, c.fkeep, c.used, c.fpart, c.hdr);
    hipLaunchKernelGGL(k_simplify_vcount, dim3(vblk), dim3(256), 0, st, c.rep, c.used, V, c.vpart, c.hdr);
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(CLEAN_SCAN_THREADS), 0, st, c.vpart, vblk, c.vbase, c.hdr, (int)SIMPLIFY_W_KEPT_VERTS);
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(CLEAN_SCAN_THREADS), 0, st, c.fpart, fblk, c.fbase, c.hdr, (int)SIMPLIFY_W_KEPT_FACES);
    hipLaunchKernelGGL(k_simplify_remap, dim3(vblk), dim3(256), 0, st, c.rep, c.used, V, c.vbase, c.remap, c.hdr);
    hipLaunchKernelGGL(k_simplify_seal, dim3(1), dim3(1), 0, st, c.hdr, (u64)SIMPLIFY_STAGE_PLANNED);
    if (int e = check_launch(what)) return e;
    u64 host[SIMPLIFY_WORDS];
    if (int e = read_simplify_header(host, c.hdr, st)) return e;
    if (host[SIMPLIFY_W_ERROR] & SIMPLIFY_ERR_FACE_ID) return fail_rule(what, KFX_E_RANGE, "a face id >= n_verts");
    if (host[SIMPLIFY_W_ERROR]) return fail_rule(what, KFX_E_RANGE, "a table probe exceeded its cap");
    out[0] = host[SIMPLIFY_W_KEPT_VERTS];
    out[1] = host[SIMPLIFY_W_KEPT_FACES];
    return 0;
}

extern "C" int kfx_mesh_simplify_emit(const void* scratch, size_t scratch_bytes, unsigned long long n_verts, unsigned long long n_faces,
                                      const unsigned long long kept[2], const float* verts, const float* norms, const float* colors,
                                      const unsigned* faces, float* verts_out, float* norms_out, float* colors_out, unsigned* faces_out,
                                      unsigned* vertex_cluster, kfx_stream stream)
{
    const char* const what = "kfx_mesh_simplify_emit";
    SimplifyCall c;
    if (int e = simplify_call(c, what, n_verts, n_faces, scratch, scratch_bytes)) return e;
    if (n_faces == 0) return 0;
    if (int e = refuse(clean_check_planned(n_verts, n_faces, kept, true), what)) return e;
    const void* const in[4] = {verts, norms, colors, faces};
    const void* const outs[4] = {verts_out, norms_out, colors_out, faces_out};
    if (int e = refuse(clean_check_filter_arrays(n_verts, n_faces, kept, in, outs, scratch, scratch_bytes), what)) return e;
    if (int e = refuse(simplify_check_map(vertex_cluster, n_verts, n_faces, kept, in, outs, scratch, scratch_bytes), what)) return e;
    const hipStream_t st = (hipStream_t)stream;
    u64 host[SIMPLIFY_WORDS];
    if (int e = read_simplify_header(host, c.hdr, st)) return e;
    if (host[SIMPLIFY_W_MAGIC] != SIMPLIFY_MAGIC || host[SIMPLIFY_W_VERTS] != n_verts || host[SIMPLIFY_W_FACES] != n_faces ||
        host[SIMPLIFY_W_STAGE] != SIMPLIFY_STAGE_PLANNED || host[SIMPLIFY_W_ERROR])
        return fail_rule(what, KFX_E_RANGE, "the scratch is not this mesh's plan");
    if (host[SIMPLIFY_W_KEPT_VERTS] != kept[0] || host[SIMPLIFY_W_KEPT_FACES] != kept[1]) return fail_rule(what, KFX_E_RANGE, "kept counts are not the plan's");
    if (kept[0] == 0 && !vertex_cluster) return 0;
    const unsigned V = (unsigned)n_verts, T = (unsigned)n_faces;
    const unsigned* const n_in = norms && norms_out ? (const unsigned*)norms : nullptr;
    const unsigned* const c_in = colors && colors_out ? (const unsigned*)colors : nullptr;
    const bool c16 = c_in && !(((uintptr_t)colors | (uintptr_t)colors_out) & 15);
    auto gather = c16 ? k_simplify_gather<true> : k_simplify_gather<false>;
    hipLaunchKernelGGL(gather, dim3(simplify_blocks_of(n_verts)), dim3(256), 0, st, c.rep, c.remap, V, (const unsigned*)verts, n_in, c_in,
                       (unsigned*)verts_out, (unsigned*)norms_out, (unsigned*)colors_out, vertex_cluster);
    if (kept[1])
        hipLaunchKernelGGL(k_simplify_faces, dim3(simplify_blocks_of(n_faces)), dim3(256), 0, st, faces, T, V, c.fkeep, c.rep, c.remap, c.fbase, faces_out);
    return check_launch(what);
}
