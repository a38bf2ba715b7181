// block_scan.h -- the workgroup scan the compactions share (mesh.hip: active cubes and triangles; bricks.hip: live bricks).
#pragma once

#include <hip/hip_runtime.h>

namespace kfx {

// inclusive scan of one value per thread over a workgroup of 64 * NW threads; returns the exclusive prefix, *total the sum
template <typename T, int NW>
__device__ __forceinline__ T block_exclusive_scan(T v, T* lds, T* total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    T base = 0, sum = 0;
    for (int i = 0; i < NW; ++i) {
        const T w = lds[i];
        if (i < wv) base += w;
        sum += w;
    }
    __syncthreads();
    *total = sum;
    return base + inc - v;
}

} // namespace kfx
