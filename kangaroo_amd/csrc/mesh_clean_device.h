// mesh_clean_device.h -- the kernels and device helpers that the passes over an indexed mesh share (mesh_clean.hip, mesh_simplify.hip):
// the error word of a scratch header, the check of the face ids, the workgroup sum and the scan of the blocks' partial counts.  Both
// headers keep their error word at CLEAN_W_ERROR and a face id >= V at bit CLEAN_ERR_FACE_ID (mesh_clean_host.h, mesh_simplify_host.h).
// The kernels have internal linkage: each unit that includes this launches its own copy.
#pragma once

#include "block_scan.h"
#include "mesh_clean_host.h"

namespace kfx {

__device__ __forceinline__ void raise(unsigned long long* hdr, unsigned long long bits)
{
    __hip_atomic_fetch_or(hdr + CLEAN_W_ERROR, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the sum of one value per thread over a workgroup of 256, in every thread
__device__ __forceinline__ unsigned block_sum(unsigned v)
{
    __shared__ unsigned lds[4];
    unsigned total;
    block_exclusive_scan<unsigned, 4>(v, lds, &total);
    return total;
}

// reads `faces` ALONE: an id >= V raises CLEAN_ERR_FACE_ID in the header
static __global__ __launch_bounds__(256) void k_clean_validate(const unsigned* __restrict__ faces, const unsigned long long n_ids, const unsigned n_verts,
                                                               unsigned long long* __restrict__ hdr)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const bool bad = i < n_ids && faces[i] >= n_verts;
    if (__ballot(bad) && (threadIdx.x & 63) == 0) raise(hdr, CLEAN_ERR_FACE_ID);
}

// one workgroup: the exclusive offsets of n blocks and their total (< 2^32: they count vertices or faces)
constexpr int CLEAN_SCAN_THREADS = 1024, CLEAN_SCAN_PER_THREAD = 8;
static __global__ __launch_bounds__(CLEAN_SCAN_THREADS) void k_clean_scan(const unsigned* __restrict__ part, const unsigned n, unsigned* __restrict__ base,
                                                                          unsigned long long* __restrict__ hdr, const int total_word)
{
    if (hdr[CLEAN_W_ERROR]) return;
    __shared__ unsigned lds[CLEAN_SCAN_THREADS / 64];
    unsigned run = 0;
    constexpr unsigned CHUNK = CLEAN_SCAN_THREADS * CLEAN_SCAN_PER_THREAD;
    for (unsigned long long c0 = 0; c0 < n; c0 += CHUNK) {
        const unsigned long long b0 = c0 + (unsigned long long)threadIdx.x * CLEAN_SCAN_PER_THREAD;
        unsigned v[CLEAN_SCAN_PER_THREAD], sum = 0;
#pragma unroll
        for (int j = 0; j < CLEAN_SCAN_PER_THREAD; ++j) {
            v[j] = b0 + j < n ? part[b0 + j] : 0u;
            sum += v[j];
        }
        unsigned total;
        unsigned ex = block_exclusive_scan<unsigned, CLEAN_SCAN_THREADS / 64>(sum, lds, &total) + run;
#pragma unroll
        for (int j = 0; j < CLEAN_SCAN_PER_THREAD; ++j) {
            if (b0 + j < n) base[b0 + j] = ex;
            ex += v[j];
        }
        run += total;
    }
    if (threadIdx.x == 0) hdr[total_word] = run;
}

} // namespace kfx
