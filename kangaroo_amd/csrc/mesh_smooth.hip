// mesh_smooth.hip -- smoothing of an indexed mesh in device memory for gfx950 (include/kfx_mesh_smooth.h): per-vertex incidence lists in
// ascending order, Laplacian / Taubin passes over them, normals from the faces.  The host rules and the per-vertex rules (rank, neighbour
// entries, flags, one pass, one normal) are mesh_smooth_host.h's.
//
// kfx_mesh_adjacency, in stream order after a memset of the header -- a counting sort of the 3T corner slots by vertex id, made stable
// afterwards:
//   k_clean_validate    (mesh_clean_device.h) reads `faces` ALONE: an id >= V raises the face-id bit in the header.  Every later kernel
//                       tests the error word before it does anything, so no id from the caller is used as an address unchecked.
//   k_adj_init          cnt[] = 0; the header's magic, V and T
//   k_adj_count         one lane per corner slot: an integer atomic add on its vertex's counter
//   k_adj_part, k_clean_scan, k_adj_start   inc_start[] by a scan of the counters; the counter becomes the segment's cursor; a vertex with
//                       more than ADJ_WIDE incidences appends itself to the wide list
//   k_adj_fill          one lane per corner slot: a position of its vertex's segment through the cursor (which position depends on
//                       arrival), its slot into tmp[]
//   k_adj_rank          one lane per corner slot of a narrow vertex: counts the smaller slots of its segment in tmp[] and writes itself
//                       at that rank into inc[] -- what inc[] holds at the end depends on the set of the segment alone
//   k_adj_flags         one lane per narrow vertex
//   k_adj_wide          a workgroup per wide vertex (a fixed grid strides over the list, whose length it reads on the device): ranks and
//                       flags with 256 lanes, so that a hub of thousands of faces costs d^2 / 256 steps, not d^2
// kfx_mesh_smooth: k_clean_validate, k_smooth_validate (reads the adjacency arrays ALONE), k_smooth_table (the neighbour entries of every
// incidence, 8 bytes, and the check that the incidence names its vertex), then one k_smooth_pass per pass, one lane per vertex: its sum
// runs over its entries in order, so the order of every float addition is fixed.  kfx_mesh_vertex_normals likewise with k_normals.
// The only atomics are integer adds and ors.  No lane waits for another; every loop runs to a bound that is fixed before it starts.
#include "host_args.h"
#include "mesh_clean_device.h"   // raise, block_sum, k_clean_validate, k_clean_scan
#include "mesh_smooth_host.h"

namespace kfx {

using u64 = unsigned long long;

constexpr unsigned ADJ_WIDE_BLOCKS = 256;   // the grid that strides over the wide list

__global__ __launch_bounds__(256) void k_adj_init(unsigned* __restrict__ cnt, const unsigned n_verts, const unsigned n_faces, u64* __restrict__ hdr)
{
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v < n_verts) cnt[v] = 0;
    if (v == 0) {
        hdr[SMOOTH_W_MAGIC] = SMOOTH_MAGIC;
        hdr[SMOOTH_W_VERTS] = n_verts;
        hdr[SMOOTH_W_FACES] = n_faces;
    }
}

__global__ __launch_bounds__(256) void k_adj_count(const unsigned* __restrict__ faces, const u64 n_ids, unsigned* cnt, const u64* __restrict__ hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s < n_ids) __hip_atomic_fetch_add(cnt + faces[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_adj_part(const unsigned* __restrict__ cnt, const unsigned n_verts, unsigned* __restrict__ vpart,
                                                  const u64* __restrict__ hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    const unsigned total = block_sum(v < n_verts ? cnt[v] : 0u);
    if (threadIdx.x == 0) vpart[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_adj_start(unsigned* __restrict__ cnt, const unsigned n_verts, const unsigned* __restrict__ vbase,
                                                   unsigned* __restrict__ inc_start, unsigned* __restrict__ wide, const u64 wide_cap, u64* hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    __shared__ unsigned lds[4];
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    const unsigned d = v < n_verts ? cnt[v] : 0u;
    unsigned total;
    const unsigned at = vbase[blockIdx.x] + block_exclusive_scan<unsigned, 4>(d, lds, &total);
    if (v >= n_verts) return;
    inc_start[v] = at;
    cnt[v] = at;
    if (v == n_verts - 1) inc_start[n_verts] = at + d;
    if (d > ADJ_WIDE) {
        const u64 pos = __hip_atomic_fetch_add(hdr + SMOOTH_W_WIDE, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (pos < wide_cap) wide[pos] = v;   // (more than 64 incidences each: at most 3T / 65 of them)
    }
}

__global__ __launch_bounds__(256) void k_adj_fill(const unsigned* __restrict__ faces, const u64 n_ids, unsigned* cursor, unsigned* __restrict__ tmp,
                                                  u64* hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_ids) return;
    const unsigned pos = __hip_atomic_fetch_add(cursor + faces[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pos < n_ids)
        tmp[pos] = (unsigned)s;
    else
        raise(hdr, SMOOTH_ERR_ADJ);   // (the cursors end where the counts put them: never raised by a correct build)
}

__global__ __launch_bounds__(256) void k_adj_rank(const unsigned* __restrict__ faces, const u64 n_ids, const unsigned* __restrict__ inc_start,
                                                  const unsigned* __restrict__ tmp, unsigned* __restrict__ inc, const u64* __restrict__ hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    const u64 s = (u64)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_ids) return;
    const unsigned v = faces[s], a = inc_start[v], d = inc_start[v + 1] - a;
    if (d > ADJ_WIDE) return;
    inc[a + adj_rank(tmp + a, d, (unsigned)s)] = (unsigned)s;
}

__global__ __launch_bounds__(256) void k_adj_flags(const unsigned* __restrict__ faces, const unsigned n_verts, const unsigned* __restrict__ inc_start,
                                                   const unsigned* __restrict__ tmp, unsigned* __restrict__ flags, const u64* __restrict__ hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    const unsigned a = inc_start[v], d = inc_start[v + 1] - a;
    if (d > ADJ_WIDE) return;
    flags[v] = d ? adj_flags(NbrFromFaces{faces, tmp + a}, d, v, 0u, 1u) : KFX_MESH_ISOLATED;
}

__global__ __launch_bounds__(256) void k_adj_wide(const unsigned* __restrict__ faces, const unsigned* __restrict__ inc_start, const unsigned* __restrict__ tmp,
                                                  const unsigned* __restrict__ wide, const u64 wide_cap, unsigned* __restrict__ inc,
                                                  unsigned* __restrict__ flags, const u64* __restrict__ hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    __shared__ unsigned bits_lds;
    const u64 listed = hdr[SMOOTH_W_WIDE];
    const u64 n = listed < wide_cap ? listed : wide_cap;
    for (u64 w = blockIdx.x; w < n; w += gridDim.x) {
        const unsigned v = wide[w], a = inc_start[v], d = inc_start[v + 1] - a;
        for (unsigned i = threadIdx.x; i < d; i += 256) {
            const unsigned s = tmp[a + i];
            inc[a + adj_rank(tmp + a, d, s)] = s;
        }
        if (flags) {
            if (threadIdx.x == 0) bits_lds = 0;
            __syncthreads();
            const unsigned bits = adj_flags(NbrFromFaces{faces, tmp + a}, d, v, threadIdx.x, 256u);
            if (bits) atomicOr(&bits_lds, bits);
            __syncthreads();
            if (threadIdx.x == 0) flags[v] = bits_lds;
            __syncthreads();
        }
    }
}

// reads the adjacency arrays ALONE: inc_start[0] == 0, ascending, inc_start[V] == 3T; every inc < 3T
__global__ __launch_bounds__(256) void k_smooth_validate(const unsigned* __restrict__ inc_start, const unsigned* __restrict__ inc, const unsigned n_verts,
                                                         const u64 n_ids, u64* __restrict__ hdr)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    bool bad = i < n_ids && inc[i] >= n_ids;
    if (i < n_verts) bad = bad || inc_start[i] > inc_start[i + 1];
    if (i == 0) bad = bad || inc_start[0] != 0 || inc_start[n_verts] != n_ids;
    if (__ballot(bad) && (threadIdx.x & 63) == 0) raise(hdr, SMOOTH_ERR_ADJ);
}

// the neighbour entries of every incidence; an incidence that does not name its vertex raises the error word
__global__ __launch_bounds__(256) void k_smooth_table(const unsigned* __restrict__ faces, const unsigned* __restrict__ inc_start,
                                                      const unsigned* __restrict__ inc, const unsigned n_verts, unsigned* __restrict__ table, u64* hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    const unsigned a = inc_start[v], d = inc_start[v + 1] - a;
    const NbrFromFaces nbr{faces, inc + a};
    bool bad = false;
    for (unsigned i = 0; i < d; ++i) {
        bad = bad || faces[inc[a + i]] != v;
        table[2 * (size_t)(a + i)] = nbr.at(2 * i);
        table[2 * (size_t)(a + i) + 1] = nbr.at(2 * i + 1);
    }
    if (bad) raise(hdr, SMOOTH_ERR_ADJ);
}

__global__ __launch_bounds__(256) void k_smooth_pass(const unsigned* __restrict__ src, unsigned* __restrict__ dst, const unsigned* __restrict__ inc_start,
                                                     const unsigned* __restrict__ table, const unsigned* __restrict__ flags, const unsigned pin_mask,
                                                     const float factor, const unsigned n_verts, const u64* __restrict__ hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    const unsigned a = inc_start[v], d = inc_start[v + 1] - a;
    const bool pinned = pin_mask && (flags[v] & pin_mask);
    unsigned out[3];
    smooth_vertex(src, v, NbrFromTable{table + 2 * (size_t)a}, d, pinned, factor, out);
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[3 * (size_t)v + k] = out[k];
}

__global__ __launch_bounds__(256) void k_smooth_copy(const unsigned* __restrict__ src, unsigned* __restrict__ dst, const u64 n_words, const u64* __restrict__ hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void k_normals(const unsigned* __restrict__ verts, const unsigned* __restrict__ faces, const unsigned* __restrict__ inc_start,
                                                 const unsigned* __restrict__ inc, const unsigned n_verts, float* __restrict__ norms_out,
                                                 const u64* __restrict__ hdr)
{
    if (hdr[SMOOTH_W_ERROR]) return;
    const unsigned v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n_verts) return;
    const unsigned a = inc_start[v], d = inc_start[v + 1] - a;
    float out[3];
    normal_vertex(verts, faces, inc + a, d, out);
#pragma unroll
    for (int k = 0; k < 3; ++k) norms_out[3 * (size_t)v + k] = out[k];
}

// ---- host side ----

static unsigned smooth_blocks_of(u64 n) { return (unsigned)((n + CLEAN_BLOCK - 1) / CLEAN_BLOCK); }

// the scratch of a call whose counts are accepted, before any HIP call
static int smooth_call(const char* what, size_t need, const void* scratch, size_t scratch_bytes)
{
    return refuse(smooth_check_scratch(need, scratch, scratch_bytes), what);
}

// the error word, once the stream's earlier work is done: 0, or the refusal it stands for
static int smooth_verdict(const char* what, const u64* hdr, hipStream_t st)
{
    if (int e = check_launch(what)) return e;
    u64 host[SMOOTH_WORDS];
    hipError_t e = hipMemcpyAsync(host, hdr, SMOOTH_WORDS * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_error((int)e, hipGetErrorString(e));
    if (host[SMOOTH_W_ERROR] & SMOOTH_ERR_FACE_ID) return fail_rule(what, KFX_E_RANGE, "a face id >= n_verts");
    if (host[SMOOTH_W_ERROR]) return fail_rule(what, KFX_E_RANGE, "inc_start / inc are not this mesh's adjacency");
    return 0;
}

// the two checks every call starts with: the header zeroed, the face ids, and (adjacency given) the adjacency arrays
static int smooth_begin(u64* hdr, const unsigned* faces, const unsigned* inc_start, const unsigned* inc, u64 n_verts, u64 n_faces, hipStream_t st)
{
    if (hipError_t e = hipMemsetAsync(hdr, 0, 256, st); e != hipSuccess) return set_error((int)e, hipGetErrorString(e));
    hipLaunchKernelGGL(k_clean_validate, dim3(smooth_blocks_of(3 * n_faces)), dim3(256), 0, st, faces, 3 * n_faces, (unsigned)n_verts, hdr);
    if (inc_start)
        hipLaunchKernelGGL(k_smooth_validate, dim3(smooth_blocks_of(3 * n_faces)), dim3(256), 0, st, inc_start, inc, (unsigned)n_verts, 3 * n_faces, hdr);
    return 0;
}

} // namespace kfx

using namespace kfx;

extern "C" size_t kfx_mesh_adjacency_scratch_bytes(unsigned long long n_verts, unsigned long long n_faces)
{
    if (clean_check_counts(n_verts, n_faces).code) return 0;
    return adj_scratch(n_verts, n_faces).bytes;
}

extern "C" size_t kfx_mesh_smooth_scratch_bytes(unsigned long long n_verts, unsigned long long n_faces)
{
    if (clean_check_counts(n_verts, n_faces).code) return 0;
    return smooth_scratch(n_verts, n_faces).bytes;
}

extern "C" size_t kfx_mesh_vertex_normals_scratch_bytes(unsigned long long n_verts, unsigned long long n_faces)
{
    if (clean_check_counts(n_verts, n_faces).code) return 0;
    return NORMALS_SCRATCH_BYTES;
}

extern "C" int kfx_mesh_adjacency(const unsigned* faces, unsigned long long n_faces, unsigned long long n_verts, unsigned* inc_start, unsigned* inc,
                                  unsigned* vertex_flags, void* scratch, size_t scratch_bytes, kfx_stream stream)
{
    const char* const what = "kfx_mesh_adjacency";
    if (int e = refuse(clean_check_counts(n_verts, n_faces), what)) return e;
    const AdjScratch s = adj_scratch(n_verts, n_faces);
    if (int e = smooth_call(what, s.bytes, scratch, scratch_bytes)) return e;
    if (n_faces == 0) return 0;
    const SmoothArray in[1] = {{faces, 12 * n_faces, false}};
    const SmoothArray out[3] = {{inc_start, 4 * (n_verts + 1), false}, {inc, 12 * n_faces, false}, {vertex_flags, 4 * n_verts, true}};
    if (int e = refuse(smooth_check_arrays(in, 1, out, 3, scratch, scratch_bytes), what)) return e;
    unsigned char* const at = (unsigned char*)scratch;
    u64* const hdr = (u64*)(at + s.hdr);
    unsigned *const cnt = (unsigned*)(at + s.cnt), *const tmp = (unsigned*)(at + s.tmp), *const wide = (unsigned*)(at + s.wide);
    unsigned *const vpart = (unsigned*)(at + s.vpart), *const vbase = (unsigned*)(at + s.vbase);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned V = (unsigned)n_verts, T = (unsigned)n_faces, vblk = (unsigned)s.vblk, sblk = smooth_blocks_of(3 * n_faces);
    const u64 n_ids = 3 * n_faces;
    if (int e = smooth_begin(hdr, faces, nullptr, nullptr, n_verts, n_faces, st)) return e;
    hipLaunchKernelGGL(k_adj_init, dim3(vblk), dim3(256), 0, st, cnt, V, T, hdr);
    hipLaunchKernelGGL(k_adj_count, dim3(sblk), dim3(256), 0, st, faces, n_ids, cnt, hdr);
    hipLaunchKernelGGL(k_adj_part, dim3(vblk), dim3(256), 0, st, cnt, V, vpart, hdr);
    hipLaunchKernelGGL(k_clean_scan, dim3(1), dim3(CLEAN_SCAN_THREADS), 0, st, vpart, vblk, vbase, hdr, (int)SMOOTH_W_TOTAL);
    hipLaunchKernelGGL(k_adj_start, dim3(vblk), dim3(256), 0, st, cnt, V, vbase, inc_start, wide, s.wide_cap, hdr);
    hipLaunchKernelGGL(k_adj_fill, dim3(sblk), dim3(256), 0, st, faces, n_ids, cnt, tmp, hdr);
    hipLaunchKernelGGL(k_adj_rank, dim3(sblk), dim3(256), 0, st, faces, n_ids, inc_start, tmp, inc, hdr);
    if (vertex_flags) hipLaunchKernelGGL(k_adj_flags, dim3(vblk), dim3(256), 0, st, faces, V, inc_start, tmp, vertex_flags, hdr);
    const unsigned wblk = (unsigned)(s.wide_cap < ADJ_WIDE_BLOCKS ? s.wide_cap : ADJ_WIDE_BLOCKS);
    hipLaunchKernelGGL(k_adj_wide, dim3(wblk), dim3(256), 0, st, faces, inc_start, tmp, wide, s.wide_cap, inc, vertex_flags, hdr);
    return smooth_verdict(what, hdr, st);
}

extern "C" int kfx_mesh_smooth(const float* verts, const unsigned* faces, unsigned long long n_faces, unsigned long long n_verts,
                               const unsigned* inc_start, const unsigned* inc, const unsigned* vertex_flags, int iterations, float lambda, float mu,
                               unsigned pin_mask, float* verts_out, void* scratch, size_t scratch_bytes, kfx_stream stream)
{
    const char* const what = "kfx_mesh_smooth";
    if (int e = refuse(clean_check_counts(n_verts, n_faces), what)) return e;
    const SmoothScratch s = smooth_scratch(n_verts, n_faces);
    if (int e = smooth_call(what, s.bytes, scratch, scratch_bytes)) return e;
    if (int e = refuse(smooth_check_params(iterations, lambda, mu), what)) return e;
    if (n_faces == 0) return 0;
    const SmoothArray in[5] = {{verts, 12 * n_verts, false}, {faces, 12 * n_faces, false}, {inc_start, 4 * (n_verts + 1), false},
                               {inc, 12 * n_faces, false}, {vertex_flags, 4 * n_verts, pin_mask == 0}};
    const SmoothArray out[1] = {{verts_out, 12 * n_verts, false}};
    if (int e = refuse(smooth_check_arrays(in, 5, out, 1, scratch, scratch_bytes), what)) return e;
    unsigned char* const at = (unsigned char*)scratch;
    u64* const hdr = (u64*)(at + s.hdr);
    unsigned *const buf = (unsigned*)(at + s.buf), *const table = (unsigned*)(at + s.table);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned V = (unsigned)n_verts, vblk = smooth_blocks_of(n_verts);
    if (int e = smooth_begin(hdr, faces, inc_start, inc, n_verts, n_faces, st)) return e;
    hipLaunchKernelGGL(k_smooth_table, dim3(vblk), dim3(256), 0, st, faces, inc_start, inc, V, table, hdr);
    const long long n_pass = mu == 0.0f ? (long long)iterations : 2ll * iterations;
    if (n_pass == 0)
        hipLaunchKernelGGL(k_smooth_copy, dim3(smooth_blocks_of(3 * n_verts)), dim3(256), 0, st, (const unsigned*)verts, (unsigned*)verts_out, 3 * n_verts, hdr);
    const unsigned* src = (const unsigned*)verts;
    for (long long k = 0; k < n_pass; ++k) {
        unsigned* const dst = (n_pass - 1 - k) % 2 == 0 ? (unsigned*)verts_out : buf;   // the last pass lands in verts_out
        const float factor = mu == 0.0f || k % 2 == 0 ? lambda : mu;
        hipLaunchKernelGGL(k_smooth_pass, dim3(vblk), dim3(256), 0, st, src, dst, inc_start, table, vertex_flags, pin_mask, factor, V, hdr);
        src = dst;
    }
    return smooth_verdict(what, hdr, st);
}

extern "C" int kfx_mesh_vertex_normals(const float* verts, const unsigned* faces, unsigned long long n_faces, unsigned long long n_verts,
                                       const unsigned* inc_start, const unsigned* inc, float* norms_out, void* scratch, size_t scratch_bytes,
                                       kfx_stream stream)
{
    const char* const what = "kfx_mesh_vertex_normals";
    if (int e = refuse(clean_check_counts(n_verts, n_faces), what)) return e;
    if (int e = smooth_call(what, NORMALS_SCRATCH_BYTES, scratch, scratch_bytes)) return e;
    if (n_faces == 0) return 0;
    const SmoothArray in[4] = {{verts, 12 * n_verts, false}, {faces, 12 * n_faces, false}, {inc_start, 4 * (n_verts + 1), false}, {inc, 12 * n_faces, false}};
    const SmoothArray out[1] = {{norms_out, 12 * n_verts, false}};
    if (int e = refuse(smooth_check_arrays(in, 4, out, 1, scratch, NORMALS_SCRATCH_BYTES), what)) return e;
    u64* const hdr = (u64*)scratch;
    const hipStream_t st = (hipStream_t)stream;
    if (int e = smooth_begin(hdr, faces, inc_start, inc, n_verts, n_faces, st)) return e;
    hipLaunchKernelGGL(k_normals, dim3(smooth_blocks_of(n_verts)), dim3(256), 0, st, (const unsigned*)verts, faces, inc_start, inc, (unsigned)n_verts,
                       norms_out, hdr);
    return smooth_verdict(what, hdr, st);
}
