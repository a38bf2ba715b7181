// debug.hip -- measurement aids, built into their own library (libkfx_debug.so, include/kfx_debug.h; it links against
// libkfx.so and is not part of the drop-in boundary): in-place read-modify-write sweeps of a TSDF volume with no
// arithmetic (the HBM ceiling of the SdfFuse access pattern on this chip), exhaustive checks of the kernels' arithmetic
// shortcuts against the hardware operations, and copies of a brick summary's tables for the tests.
#include "kfx_device.h"
#include "sampling.h"
#include "../../include/kfx_debug.h"

namespace kfx {

// variant 0: linear grid-stride float4 sweep over the contiguous span
__global__ __launch_bounds__(256) void k_rmw_linear(float4* __restrict__ base, size_t n4)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 c = base[i];
        c.y += 1.0f;
        c.w += 1.0f;
        base[i] = c;
    }
}

// variant 1: the tiled fuse kernel's mapping (64 x 8 x ZC brick, 2 voxels per lane, z-march)
template <int ZC>
__global__ __launch_bounds__(256) void k_rmw_brick(unsigned char* vptr, size_t pitch, size_t img_pitch, int X, int Y, int Z)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int x0 = (blockIdx.x * 32 + (lane & 31)) * 2;
    const int y = blockIdx.y * 8 + wv * 2 + (lane >> 5);
    const int zbeg = blockIdx.z * ZC, zend = min(zbeg + ZC, Z);
    if (x0 >= X || y >= Y) return;
    unsigned char* cell = vptr + (size_t)zbeg * img_pitch + (size_t)y * pitch + (size_t)x0 * 8;
    for (int z = zbeg; z < zend; ++z, cell += img_pitch) {
        float4 c = *reinterpret_cast<const float4*>(cell);
        c.y += 1.0f;
        c.w += 1.0f;
        *reinterpret_cast<float4*>(cell) = c;
    }
}

// variant 2: the first kernels' mapping (128 x 4 x ZC brick: one wave = one 1 KiB row segment)
template <int ZC>
__global__ __launch_bounds__(256) void k_rmw_rows(unsigned char* vptr, size_t pitch, size_t img_pitch, int X, int Y, int Z)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = (blockIdx.x * 64 + lane) * 2;
    const int y = blockIdx.y * 4 + wv;
    const int zbeg = blockIdx.z * ZC, zend = min(zbeg + ZC, Z);
    if (x0 >= X || y >= Y) return;
    unsigned char* cell = vptr + (size_t)zbeg * img_pitch + (size_t)y * pitch + (size_t)x0 * 8;
    for (int z = zbeg; z < zend; ++z, cell += img_pitch) {
        float4 c = *reinterpret_cast<const float4*>(cell);
        c.y += 1.0f;
        c.w += 1.0f;
        *reinterpret_cast<float4*>(cell) = c;
    }
}

// variant 3: z-march, but each workgroup walks the WHOLE z range of its (x,y) footprint
__global__ __launch_bounds__(256) void k_rmw_column(unsigned char* vptr, size_t pitch, size_t img_pitch, int X, int Y, int Z)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = (blockIdx.x * 64 + lane) * 2;
    const int y = blockIdx.y * 4 + wv;
    if (x0 >= X || y >= Y) return;
    unsigned char* cell = vptr + (size_t)y * pitch + (size_t)x0 * 8;
    for (int z = 0; z < Z; ++z, cell += img_pitch) {
        float4 c = *reinterpret_cast<const float4*>(cell);
        c.y += 1.0f;
        c.w += 1.0f;
        *reinterpret_cast<float4*>(cell) = c;
    }
}

// generic: WX waves side by side along x (each 128 voxels = 1 KiB), WY rows, ZC slices, optional
// nontemporal accesses; WX*WY = 4 waves
typedef float v4f_dbg __attribute__((ext_vector_type(4)));
template <int WX, int WY, int ZC, bool NT>
__global__ __launch_bounds__(256) void k_rmw_gen(unsigned char* vptr, size_t pitch, size_t img_pitch, int X, int Y, int Z)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x0 = ((blockIdx.x * WX + (wv % WX)) * 64 + lane) * 2;
    const int y = blockIdx.y * WY + (wv / WX);
    const int zbeg = blockIdx.z * ZC, zend = min(zbeg + ZC, Z);
    if (x0 >= X || y >= Y) return;
    unsigned char* cell = vptr + (size_t)zbeg * img_pitch + (size_t)y * pitch + (size_t)x0 * 8;
    for (int z = zbeg; z < zend; ++z, cell += img_pitch) {
        v4f_dbg c;
        if constexpr (NT) c = __builtin_nontemporal_load(reinterpret_cast<const v4f_dbg*>(cell));
        else c = *reinterpret_cast<const v4f_dbg*>(cell);
        c.y += 1.0f;
        c.w += 1.0f;
        if constexpr (NT) __builtin_nontemporal_store(c, reinterpret_cast<v4f_dbg*>(cell));
        else *reinterpret_cast<v4f_dbg*>(cell) = c;
    }
}

// exhaustive check of div_uniform against the hardware division: every numerator bit pattern for one divisor
__global__ __launch_bounds__(256) void k_div_uniform_check(float b, float inv, unsigned long long* __restrict__ out)
{
    unsigned long long bad = 0, tested = 0;
    const unsigned stride = gridDim.x * blockDim.x;
    unsigned bits = blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned it = 0; it < (1u << 16); ++it, bits += stride) { // grid = 2^16 threads: 2^16 iterations cover 2^32 patterns
        const float a = __uint_as_float(bits);
        if (!div_uniform_safe(a)) continue;
        const float want = a / b;
        const float got = div_uniform(a, b, inv);
        tested += 1;
        bad += (__float_as_uint(want) != __float_as_uint(got)) ? 1 : 0;
    }
    atomicAdd(out, bad);
    atomicAdd(out + 1, tested);
}

// div_core / rcp_nr against the hardware IEEE division.  Thread t sweeps divisor significands (every 2^23 of them
// across the grid) in each of a set of binades and pairs each with numerators from a counter-based generator
// (splitmix-style hash): random significands in random binades of [2^-60, 2^60], plus the awkward ones (all ones, one ulp
// above / below a power of two) and exact zeros.  A signed-zero quotient counts as equal to the other zero.
__device__ __forceinline__ unsigned hash32(unsigned long long x)
{
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return (unsigned)((x ^ (x >> 31)) >> 16);
}
__global__ __launch_bounds__(256) void k_div_core_check(unsigned seed, int per_divisor, unsigned long long* __restrict__ out)
{
    const int bexp[] = {-40, -20, -3, -1, 0, 1, 2, 10, 20, 40};
    unsigned long long bad = 0, tested = 0;
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
    for (unsigned m = tid; m < (1u << 23); m += stride) {
        for (int be = 0; be < 10; ++be) {
            const unsigned bbits = ((unsigned)(127 + bexp[be]) << 23) | m | ((m & 1u) << 31); // alternate signs
            const float b = __uint_as_float(bbits);
            const float y = rcp_nr(b);
            for (int k = 0; k < per_divisor; ++k) {
                const unsigned h = hash32(((unsigned long long)seed << 40) ^ ((unsigned long long)m << 8) ^ (unsigned)(be * 64 + k));
                unsigned am = h & 0x7fffffu;
                const int sel = (h >> 23) & 15;
                if (sel == 0) am = 0x7fffffu;
                else if (sel == 1) am = 0u;
                else if (sel == 2) am = 1u;
                else if (sel == 3) am = 0x7ffffeu;
                const int ae = (int)((h >> 27) % 121u) - 60;
                unsigned abits = ((unsigned)(127 + ae) << 23) | am | (h & 0x80000000u);
                if (k == 0) abits = h & 0x80000000u; // +-0
                const float a = __uint_as_float(abits);
                const float want = a / b;
                const float got = div_core(a, b, y);
                tested += 1;
                const bool same = __float_as_uint(want) == __float_as_uint(got) || (want == 0.0f && got == 0.0f);
                bad += same ? 0 : 1;
            }
        }
    }
    atomicAdd(out, bad);
    atomicAdd(out + 1, tested);
}

// sqrt_core against sqrtf for every float in [2^-80, 2^80]
__global__ __launch_bounds__(256) void k_sqrt_core_check(unsigned long long* __restrict__ out)
{
    unsigned long long bad = 0, tested = 0;
    const unsigned lo = (unsigned)(127 - 80) << 23, hi = (unsigned)(127 + 80) << 23;
    const unsigned stride = gridDim.x * blockDim.x;
    for (unsigned long long bits = (unsigned long long)lo + blockIdx.x * blockDim.x + threadIdx.x; bits <= hi; bits += stride) {
        const float x = __uint_as_float((unsigned)bits);
        tested += 1;
        bad += (__float_as_uint(sqrtf(x)) != __float_as_uint(sqrt_core(x))) ? 1 : 0;
    }
    atomicAdd(out, bad);
    atomicAdd(out + 1, tested);
}

// wave_xor_combine (DPP quad permutes, v_permlane16_swap / v_permlane32_swap) against __shfl_xor for the four lane
// distances, min and max, on pseudo-random lane values: out[0] += mismatching lanes, out[1] += lanes tested
__global__ __launch_bounds__(256) void k_wave_xor_check(unsigned seed, unsigned long long* __restrict__ out)
{
    unsigned s = seed ^ (blockIdx.x * 256u + threadIdx.x) * 2654435761u;
    unsigned long long bad = 0, tested = 0;
    const auto fmin2 = [](float a, float b) { return fminf(a, b); };
    const auto fmax2 = [](float a, float b) { return fmaxf(a, b); };
    for (int it = 0; it < 64; ++it) {
        s = s * 1664525u + 1013904223u;
        const float x = (float)(int)(s >> 8) * (1.0f / 8388608.0f) - 1.0f;
        const float r[8] = {wave_xor_combine<1>(x, fmin2), wave_xor_combine<2>(x, fmin2), wave_xor_combine<16>(x, fmin2), wave_xor_combine<32>(x, fmin2),
                            wave_xor_combine<1>(x, fmax2), wave_xor_combine<2>(x, fmax2), wave_xor_combine<16>(x, fmax2), wave_xor_combine<32>(x, fmax2)};
        const int off[4] = {1, 2, 16, 32};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float o = __shfl_xor(x, off[k], 64);
            bad += (__float_as_uint(r[k]) != __float_as_uint(fminf(x, o))) ? 1 : 0;
            bad += (__float_as_uint(r[4 + k]) != __float_as_uint(fmaxf(x, o))) ? 1 : 0;
            tested += 2;
        }
    }
    atomicAdd(out, bad);
    atomicAdd(out + 1, tested);
}

} // namespace kfx

using namespace kfx;

extern "C" int kfx_debug_wave_xor_check(unsigned seed, unsigned long long* d_out, kfx_stream stream)
{
    if (!d_out) return set_error(KFX_E_NULL, "kfx_debug_wave_xor_check");
    hipLaunchKernelGGL(k_wave_xor_check, dim3(64), dim3(256), 0, (hipStream_t)stream, seed, d_out);
    return check_launch("kfx_debug_wave_xor_check");
}

extern "C" int kfx_debug_div_core_check(unsigned seed, int per_divisor, unsigned long long* d_out, kfx_stream stream)
{
    if (!d_out) return set_error(KFX_E_NULL, "kfx_debug_div_core_check");
    if (per_divisor < 1 || per_divisor > 64) return set_error(KFX_E_RANGE, "kfx_debug_div_core_check: per_divisor in [1, 64]");
    hipLaunchKernelGGL(k_div_core_check, dim3(4096), dim3(256), 0, (hipStream_t)stream, seed, per_divisor, d_out);
    return check_launch("kfx_debug_div_core_check");
}

extern "C" int kfx_debug_sqrt_core_check(unsigned long long* d_out, kfx_stream stream)
{
    if (!d_out) return set_error(KFX_E_NULL, "kfx_debug_sqrt_core_check");
    hipLaunchKernelGGL(k_sqrt_core_check, dim3(4096), dim3(256), 0, (hipStream_t)stream, d_out);
    return check_launch("kfx_debug_sqrt_core_check");
}

extern "C" int kfx_debug_div_uniform_check(float b, unsigned long long* d_out, kfx_stream stream)
{
    if (!d_out) return set_error(KFX_E_NULL, "kfx_debug_div_uniform_check");
    if (!div_uniform_safe_host(b)) return set_error(KFX_E_RANGE, "kfx_debug_div_uniform_check: divisor outside [2^-40, 2^40]");
    hipLaunchKernelGGL(k_div_uniform_check, dim3(256), dim3(256), 0, (hipStream_t)stream, b, 1.0f / b, d_out);
    return check_launch("kfx_debug_div_uniform_check");
}

extern "C" int kfx_debug_rmw(const kfx_volume* vol, int variant, kfx_stream stream)
{
    if (!vol || !vol->ptr) return set_error(KFX_E_NULL, "kfx_debug_rmw");
    hipStream_t s = (hipStream_t)stream;
    const int X = (int)vol->w, Y = (int)vol->h, Z = (int)vol->d;
    unsigned char* p = (unsigned char*)vol->ptr;
    switch (variant) {
    case 0: {
        const size_t n4 = ((vol->d - 1) * vol->img_pitch + (vol->h - 1) * vol->pitch + vol->w * 8) / 16;
        hipLaunchKernelGGL(k_rmw_linear, dim3(256 * 8), dim3(256), 0, s, (float4*)p, n4);
        break;
    }
    case 1: hipLaunchKernelGGL(k_rmw_brick<16>, dim3(ceil_div(X, 64), ceil_div(Y, 8), ceil_div(Z, 16)), dim3(256), 0, s, p, vol->pitch, vol->img_pitch, X, Y, Z); break;
    case 2: hipLaunchKernelGGL(k_rmw_rows<16>, dim3(ceil_div(X, 128), ceil_div(Y, 4), ceil_div(Z, 16)), dim3(256), 0, s, p, vol->pitch, vol->img_pitch, X, Y, Z); break;
    case 3: hipLaunchKernelGGL(k_rmw_column, dim3(ceil_div(X, 128), ceil_div(Y, 4), 1), dim3(256), 0, s, p, vol->pitch, vol->img_pitch, X, Y, Z); break;
    case 4: hipLaunchKernelGGL(k_rmw_brick<64>, dim3(ceil_div(X, 64), ceil_div(Y, 8), ceil_div(Z, 64)), dim3(256), 0, s, p, vol->pitch, vol->img_pitch, X, Y, Z); break;
    case 5: hipLaunchKernelGGL(k_rmw_rows<4>, dim3(ceil_div(X, 128), ceil_div(Y, 4), ceil_div(Z, 4)), dim3(256), 0, s, p, vol->pitch, vol->img_pitch, X, Y, Z); break;
#define GEN(ID, WX, WY, ZC, NT) \
    case ID: hipLaunchKernelGGL((k_rmw_gen<WX, WY, ZC, NT>), dim3(ceil_div(X, 128 * WX), ceil_div(Y, WY), ceil_div(Z, ZC)), dim3(256), 0, s, p, vol->pitch, vol->img_pitch, X, Y, Z); break;
    GEN(10, 4, 1, 16, false)
    GEN(11, 2, 2, 16, false)
    GEN(12, 1, 4, 16, false)
    GEN(13, 1, 4, 16, true)
    GEN(14, 4, 1, 16, true)
    GEN(15, 1, 4, 1, false)
    GEN(16, 1, 4, 64, false)
    GEN(17, 4, 1, 4, false)
    GEN(18, 2, 2, 16, true)
#undef GEN
    default: return set_error(KFX_E_RANGE, "kfx_debug_rmw: variant");
    }
    return check_launch("kfx_debug_rmw");
}

// the count the last table build issued has published (-1: it has not yet; -2: no build so far, or no ring)
static int last_published(const kfx_sdf_summary* s)
{
    if (!s->h_skippable || !s->builds) return -2;
    const uint64_t v = __atomic_load_n(s->h_skippable + summary_ring_index(s->builds - 1), __ATOMIC_ACQUIRE);
    return summary_ring_slot_stamp(v) == summary_ring_stamp(s->builds - 1) ? summary_ring_slot_count(v) : -1;
}

// test / diagnostics aid (include/kfx_debug.h): copies of R (float4 per brick) and of the class tables built for (tol, vref,
// fine_shift) into caller buffers
extern "C" int kfx_debug_summary_export(kfx_sdf_summary* s, float tol, float vref, int fine_shift, void* R_out, void* C_out, int dims_out[12],
                                        kfx_stream stream)
{
    if (!s || !dims_out) return set_error(KFX_E_NULL, "kfx_debug_summary_export: null argument");
    if (fine_shift < 3 || fine_shift > 5) return set_error(KFX_E_RANGE, "kfx_debug_summary_export: fine_shift in [3, 5]");
    ClassView cv;
    summary_class_layout(s, fine_shift, cv);
    dims_out[0] = s->nbx; dims_out[1] = s->nby; dims_out[2] = s->nbz;
    dims_out[3] = cv.fine.first; dims_out[4] = cv.fine.rw; dims_out[5] = cv.fine.ny;
    dims_out[6] = cv.coarse.first; dims_out[7] = cv.coarse.rw; dims_out[8] = cv.coarse.ny;
    dims_out[9] = cv.words; dims_out[10] = s->n_coarse; dims_out[11] = last_published(s);
    const size_t n = (size_t)s->nbx * s->nby * s->nbz;
    hipStream_t st = (hipStream_t)stream;
    if (R_out && hipMemcpyAsync(R_out, s->R, n * sizeof(float4), hipMemcpyDeviceToDevice, st) != hipSuccess) return set_error(KFX_E_RANGE, "kfx_debug_summary_export: copy");
    if (C_out) {
        if (int e = summary_classes_prepare(s, tol, vref, fine_shift, st)) return e;
        if (hipMemcpyAsync(C_out, s->C, (size_t)cv.words * sizeof(unsigned), hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return set_error(KFX_E_RANGE, "kfx_debug_summary_export: copy");
        dims_out[11] = last_published(s);   // (the build has finished: its count is published)
    }
    return 0;
}

extern "C" int kfx_debug_summary_conditional_builds(kfx_sdf_summary* s, int out[2], kfx_stream stream)
{
    if (!s || !out) return set_error(KFX_E_NULL, "kfx_debug_summary_conditional_builds: null argument");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(out, s->d_count + 3, 2 * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return set_error(KFX_E_RANGE, "kfx_debug_summary_conditional_builds: copy");
    return 0;
}

extern "C" int kfx_debug_summary_top_levels(kfx_sdf_summary* s, int fine_shift, void* top_out, int dims_out[12], unsigned long long* launches_out, kfx_stream stream)
{
    if (!s || !dims_out) return set_error(KFX_E_NULL, "kfx_debug_summary_top_levels: null argument");
    if (fine_shift < 3 || fine_shift > 5) return set_error(KFX_E_RANGE, "kfx_debug_summary_top_levels: fine_shift in [3, 5]");
    ClassView cv;
    summary_class_layout(s, fine_shift, cv);
    cv.nx5 = ceil_div(s->w, 32); cv.nz5 = ceil_div(s->d, 32);
    ClassLevel l6, l7;
    int w6, w7;
    summary_top_layout(cv, l6, l7, w6, w7);
    const int nx6 = (cv.nx5 + 1) >> 1, nz6 = (cv.nz5 + 1) >> 1;
    dims_out[0] = l6.first - cv.words; dims_out[1] = l6.rw; dims_out[2] = l6.ny; dims_out[3] = nx6; dims_out[4] = nz6; dims_out[5] = w6;
    dims_out[6] = l7.first - cv.words; dims_out[7] = l7.rw; dims_out[8] = l7.ny; dims_out[9] = (nx6 + 1) >> 1; dims_out[10] = (nz6 + 1) >> 1; dims_out[11] = w7;
    if (launches_out) *launches_out = s->launches;
    if (top_out) {
        if (s->c_shift != fine_shift) return set_error(KFX_E_RANGE, "kfx_debug_summary_top_levels: the tables held were built for another fine level");
        hipStream_t st = (hipStream_t)stream;
        if (hipMemcpyAsync(top_out, s->C + cv.words, (size_t)(w6 + w7) * sizeof(unsigned), hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return set_error(KFX_E_RANGE, "kfx_debug_summary_top_levels: copy");
    }
    return 0;
}

extern "C" int kfx_debug_fuse_keep(const kfx_sdf_summary* s, int out[3], unsigned char* kept, int n_rows)
{
    if (!s || !out) return set_error(KFX_E_NULL, "kfx_debug_fuse_keep: null argument");
    out[0] = s->keep_stride; out[1] = s->keep_row0; out[2] = s->keep_rows;
    for (int r = 0; kept && r < n_rows; ++r)
        kept[r] = (r >= s->keep_row0 && r < s->keep_row0 + s->keep_rows && keep_row(r, s->keep_stride)) ? 1 : 0;
    return 0;
}
