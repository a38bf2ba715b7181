// kfx_device.h -- shared device-side helpers for the gfx950 kernels.
//
// Numerics contract ("exact" build): this translation unit is compiled with
// -ffp-contract=off and HIP's default correctly rounded fp32 divide/sqrt, and
// every expression keeps the reference's operand order and association, so the
// kernels are bit-comparable with the CPU oracle (oracle/kfx_oracle.c).
// Reference citations are paths inside the reference tree.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/kfx.h"
#include "../../include/kfx_extras.h"
#include "../../include/kfx_summary_h.h"
#include "../../include/kfx_color.h"
#include "summary_ring_host.h"

namespace kfx {

struct V3 { float x, y, z; };

__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return V3{a.x * s, a.y * s, a.z * s}; }
// float3 / float3 is a true division (CUDA_SDK/cutil_math.h:354-357)
__device__ __forceinline__ V3 div_cw(V3 a, V3 b) { return V3{a.x / b.x, a.y / b.y, a.z / b.z}; }
// float3 / float is multiply-by-reciprocal (cutil_math.h:358-362)
__device__ __forceinline__ V3 div_s(V3 a, float s) { const float inv = 1.0f / s; return a * inv; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float length(V3 a) { return sqrtf(dot(a, a)); }
// lerp = a + t*(b-a) (cutil_math.h:80-83, :375-378)
__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }
__device__ __forceinline__ V3 lerp(V3 a, V3 b, float t) { return a + (b - a) * t; }
// clamp = fmaxf(a, fminf(f, b)) (cutil_math.h:86-89)
__device__ __forceinline__ float clampf(float f, float a, float b) { return fmaxf(a, fminf(f, b)); }

// a / b for a divisor that is uniform over the launch, with inv = 1.0f / b computed once on the host (IEEE, correctly
// rounded).  q0 = RN(a * inv) is within one ulp of the quotient, r = a - b * q0 is exact in an FMA, and RN(q0 + r * inv)
// is then the correctly rounded quotient (Markstein's correction step) -- the same float the IEEE division returns, as
// long as nothing over- or underflows: callers use it for |a|, |b| in [2^-40, 2^40] (div_uniform_safe) and take the
// hardware division otherwise.  Three instructions instead of the twelve of v_div_scale / v_rcp / fma... / v_div_fixup;
// checked exhaustively against the hardware division over all 2^32 numerators for a set of divisors
// (kfx_debug_div_uniform_check, tests/test_gpu_parity.py).
__device__ __forceinline__ float div_uniform(float a, float b, float inv)
{
    const float q0 = a * inv;
    const float r = __builtin_fmaf(-b, q0, a);
    return __builtin_fmaf(r, inv, q0);
}
__device__ __forceinline__ bool div_uniform_safe(float a) { return fabsf(a) < 0x1p40f && fabsf(a) > 0x1p-40f; }
inline bool div_uniform_safe_host(float b) { const float m = b < 0 ? -b : b; return m < 0x1p40f && m > 0x1p-40f; }

// ---- IEEE quotients and square roots without the range-scaling wrapper ---------------------------------------------
// hipcc expands a correctly rounded fp32 a / b into v_div_scale x2, v_rcp, a Newton step on the reciprocal, a quotient
// with two residual corrections, v_div_fmas and v_div_fixup: eleven instructions, five of them of the slow class (measured
// on MI355X, scripts/ubench/valu_rate.hip: v_div_scale / v_div_fmas / v_div_fixup 5.1 cycles, v_rcp 8.8, v_fma 3.3 per
// wave-instruction).  v_div_scale only rescales operands whose exponents are extreme and v_div_fixup only patches
// zero / infinity / NaN operands; in between, the expansion is exactly rcp_nr + div_core below (multiplying by a power of
// two commutes with every rounding when nothing over- or underflows), so for |b| in [2^-40, 2^40] and a = 0 or |a| in
// [2^-60, 2^60] div_core(a, b, rcp_nr(b)) IS the IEEE quotient (up to the sign of a zero result) -- and the refined
// reciprocal can be shared by several numerators.  Checked against the hardware division on the GPU
// (kfx_debug_div_core_check, tests/test_gpu_parity.py).
__device__ __forceinline__ float rcp_nr(float b)
{
    const float y0 = __builtin_amdgcn_rcpf(b);
    const float e = __builtin_fmaf(-b, y0, 1.0f);
    return __builtin_fmaf(e, y0, y0);
}
__device__ __forceinline__ float div_core(float a, float b, float y)
{
    const float q0 = a * y;
    const float r0 = __builtin_fmaf(-b, q0, a);
    const float q1 = __builtin_fmaf(r0, y, q0);
    const float r1 = __builtin_fmaf(-b, q1, a);
    return __builtin_fmaf(r1, y, q1);
}
// Correctly rounded sqrtf for x in [2^-80, 2^80]: the reciprocal-square-root iteration LLVM itself uses for IEEE sqrt
// when denormals need no care (one v_rsq_f32 and seven multiply-adds; the denormal-safe expansion hipcc emits here is
// v_sqrt_f32 plus fifteen instructions, nine of them of the slow class).  Compared with sqrtf over every float of that
// range on the GPU (kfx_debug_sqrt_core_check).
__device__ __forceinline__ float sqrt_core(float x)
{
    const float r = __builtin_amdgcn_rsqf(x);
    float s = x * r;
    float h = r * 0.5f;
    const float e = __builtin_fmaf(-h, s, 0.5f);
    h = __builtin_fmaf(h, e, h);
    s = __builtin_fmaf(s, e, s);
    const float d = __builtin_fmaf(-s, s, x);
    return __builtin_fmaf(d, h, s);
}

// A wave-uniform value the compiler would keep in a scalar register, moved to a vector register for good.  On gfx950 any
// VALU instruction with an SGPR source issues at the 5-cycle rate of the "slow" class instead of 3.3 cycles (measured:
// v_fma / v_mul / v_add / v_fmac with one SGPR operand 5.1 cycles per wave-instruction against 3.3-3.4 all-VGPR,
// scripts/ubench/valu_rate.hip), so the operands of an issue-bound inner loop belong in VGPRs even when they are uniform.
template <typename T>
__device__ __forceinline__ T in_vgpr(T x)
{
    asm volatile("" : "+v"(x));
    return x;
}

// op(x[lane], x[lane ^ OFF]) for OFF in {1, 2, 16, 32} without the LDS crossbar of __shfl_xor (ds_bpermute): DPP quad
// permutes within 4 lanes; v_permlane16_swap / v_permlane32_swap (gfx950) exchange odd and even rows / the two halves of a
// wave -- called with both operands equal they return (even-side value, odd-side value) in every lane, which is all a
// commutative op needs.
template <int OFF, typename F>
__device__ __forceinline__ float wave_xor_combine(float x, F op)
{
    static_assert(OFF == 1 || OFF == 2 || OFF == 16 || OFF == 32, "lane distance");
    const unsigned u = __float_as_uint(x);
    if constexpr (OFF == 1 || OFF == 2) {
        const int o = __builtin_amdgcn_update_dpp(0, (int)u, OFF == 1 ? 0xB1 : 0x4E, 0xF, 0xF, true); // quad_perm [1,0,3,2] / [2,3,0,1]
        return op(x, __uint_as_float((unsigned)o));
    } else if constexpr (OFF == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        return op(__uint_as_float(r[0]), __uint_as_float(r[1]));
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        return op(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
}


// op over the 8 lanes {8 k .. 8 k + 7} a lane belongs to, result in all of them: two quad permutes and DPP's row_half_mirror (lane i <->
// lane 7 - i of the half row, which pairs the two quads) -- three VALU instructions per value, no LDS
template <typename F>
__device__ __forceinline__ float wave8_combine(float x, F op)
{
    x = wave_xor_combine<1>(x, op);
    x = wave_xor_combine<2>(x, op);
    const int o = __builtin_amdgcn_update_dpp(0, (int)__float_as_uint(x), 0x141, 0xF, 0xF, true);   // row_half_mirror
    return op(x, __uint_as_float((unsigned)o));
}

// op over the 64 lanes of a wave, result in all of them: the __shfl_xor butterfly (ds_bpermute), for values of any 32-bit type
template <typename T, typename F>
__device__ __forceinline__ T wave_combine(T x, F op)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = op(x, __shfl_xor(x, off, 64));
    return x;
}

// op over the NW waves of a workgroup, in two halves with the caller's barrier between them: block_put leaves the wave's value
// in s[wv] (its lanes combined first), block_get combines s[0 .. NW) (adjacent pairs first).
template <typename F>
__device__ __forceinline__ void block_put(float* s, int wv, float x, F op)
{
    x = wave_combine(x, op);
    if ((threadIdx.x & 63) == 0) s[wv] = x;
}
template <int NW, typename F>
__device__ __forceinline__ float block_get(const float* s, F op)
{
    static_assert(NW >= 2 && (NW & (NW - 1)) == 0, "a power of two waves");
    float v[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) v[k] = s[k];
#pragma unroll
    for (int n = NW / 2; n > 0; n >>= 1)
#pragma unroll
        for (int k = 0; k < n; ++k) v[k] = op(v[2 * k], v[2 * k + 1]);
    return v[0];
}
struct FMin { __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); } };
struct FMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

// Row-major 3x4 pose, roo::Mat<float,3,4> (Mat.h:33-163)
struct Pose { float m[12]; };
// ImageIntrinsics {fu, fv, u0, v0} (ImageIntrinsics.h:51-200)
struct Intr { float fu, fv, u0, v0; };

// T * p (MatUtils.h:117-125)
__device__ __forceinline__ V3 se3_mul(const Pose& T, V3 p)
{
    return V3{T.m[0] * p.x + T.m[1] * p.y + T.m[2] * p.z + T.m[3],
              T.m[4] * p.x + T.m[5] * p.y + T.m[6] * p.z + T.m[7],
              T.m[8] * p.x + T.m[9] * p.y + T.m[10] * p.z + T.m[11]};
}
// mulSO3 (MatUtils.h:147-155)
__device__ __forceinline__ V3 so3_mul(const Pose& T, V3 r)
{
    return V3{T.m[0] * r.x + T.m[1] * r.y + T.m[2] * r.z,
              T.m[4] * r.x + T.m[5] * r.y + T.m[6] * r.z,
              T.m[8] * r.x + T.m[9] * r.y + T.m[10] * r.z};
}
// mulSO3inv (MatUtils.h:177-185)
__device__ __forceinline__ V3 so3_mul_inv(const Pose& T, V3 r)
{
    return V3{T.m[0] * r.x + T.m[4] * r.y + T.m[8] * r.z,
              T.m[1] * r.x + T.m[5] * r.y + T.m[9] * r.z,
              T.m[2] * r.x + T.m[6] * r.y + T.m[10] * r.z};
}

// Device view of a pitched image.
struct ImgView {
    const unsigned char* ptr;
    size_t pitch;
    int w, h;
};
template <typename T>
__device__ __forceinline__ const T* row(const ImgView& im, size_t y)
{
    return reinterpret_cast<const T*>(im.ptr + y * im.pitch);
}

// Device view of the rendering trio -- depth (float), normals (float4), shading image (float) -- and the size of the launch that
// reads or writes it (raycast_ray.h: ray_out finds a pixel's three addresses in it, as in a RayParams)
struct RenderImages { unsigned char *dptr, *nptr, *iptr; size_t dpitch, npitch, ipitch; int w, h; };

// Device view of BoundedVolume<SDF_t>.
struct VolView {
    unsigned char* ptr;
    size_t pitch, img_pitch;
    int w, h, d;
    V3 bmin, bmax;
};

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// ---- a per-pixel launch and a depth pixel's geometry: one definition each ---------------------------------------------
// Workgroups of 256 = PIX_W x PIX_H pixels, a wave per image row (host_args.h: pixel_grid is the grid): the thread's pixel, and for a
// kernel that also works across the lanes of its row the thread's lane (its pixel's column in the tile) and wave (its row)
constexpr int PIX_W = 64, PIX_H = 4;
__device__ __forceinline__ void pixel_xy(int& u, int& v, int& lane, int& wv)
{
    lane = threadIdx.x % PIX_W;
    wv = threadIdx.x / PIX_W;
    u = blockIdx.x * PIX_W + lane;
    v = blockIdx.y * PIX_H + wv;
}
__device__ __forceinline__ void pixel_xy(int& u, int& v)
{
    int lane, wv;
    pixel_xy(u, v, lane, wv);
}
// KernDepthToVbo (cu_depth_tools.cu:59-70): Unproject(u, v, kz) (ImageIntrinsics.h:127-131) of a pixel whose depth is kz, w = 1
__device__ __forceinline__ float4 depth_vertex(const Intr& K, float kz, int u, int v)
{
    return make_float4(kz * ((float)u - K.u0) / K.fu, kz * ((float)v - K.v0) / K.fv, kz, 1.0f);
}
// KernNormalsFromVbo (cu_normals.cu:12-38): the vertices of a pixel, of its right and of its lower neighbour
__device__ __forceinline__ float4 vertex_normal(float4 Vc, float4 Vr, float4 Vu)
{
    const V3 a = v3(Vr.x - Vc.x, Vr.y - Vc.y, Vr.z - Vc.z);
    const V3 b = v3(Vu.x - Vc.x, Vu.y - Vc.y, Vu.z - Vc.z);
    const V3 axb = v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
    const float mag = length(axb);
    return make_float4(-axb.x / mag, -axb.y / mag, -axb.z / mag, 1.0f);
}
// KernBoxHalfIgnoreInvalid<float,float,float> (cu_resample.cu:89-111): mean of the finite samples of a 2 x 2 block, NaN if
// none; samples are added in the order tl, tr, bl, br
__device__ __forceinline__ float box_half(float tl, float tr, float bl, float br)
{
    int n = 0;
    float sum = 0;
    if (isfinite(tl)) { sum += tl; n++; }
    if (isfinite(tr)) { sum += tr; n++; }
    if (isfinite(bl)) { sum += bl; n++; }
    if (isfinite(br)) { sum += br; n++; }
    return n > 0 ? (sum / n) : __builtin_nanf("");
}
// Image<uchar3>::GetBilinear<float3> (sampling.h lerp(uchar3...): integer difference, converted, times t, plus the first
// value; rows blended as float3) of an RGB image at (pu, pv), at least one pixel inside it
struct __attribute__((packed)) Rgb3 { unsigned char x, y, z; };
__device__ __forceinline__ V3 rgb_bilinear(const unsigned char* ptr, size_t pitch, float pu, float pv)
{
    const float ix = floorf(pu), iy = floorf(pv);
    const float fx = pu - ix, fy = pv - iy;
    const Rgb3* bl = reinterpret_cast<const Rgb3*>(ptr + (size_t)iy * pitch) + (size_t)ix;
    const Rgb3* tl = reinterpret_cast<const Rgb3*>(ptr + (size_t)(iy + 1) * pitch) + (size_t)ix;
    const Rgb3 b0 = bl[0], b1 = bl[1], t0 = tl[0], t1 = tl[1];
    const V3 lo = v3((float)b0.x + fx * (float)((int)b1.x - (int)b0.x), (float)b0.y + fx * (float)((int)b1.y - (int)b0.y),
                     (float)b0.z + fx * (float)((int)b1.z - (int)b0.z));
    const V3 hi = v3((float)t0.x + fx * (float)((int)t1.x - (int)t0.x), (float)t0.y + fx * (float)((int)t1.y - (int)t0.y),
                     (float)t0.z + fx * (float)((int)t1.z - (int)t0.z));
    return v3(lo.x + fy * (hi.x - lo.x), lo.y + fy * (hi.y - lo.y), lo.z + fy * (hi.z - lo.z));
}
// The packed texel image of the tiled SdfFuse kernels (fuse.hip; its geometry: host_args.h, tex_layout), written by a pixel_xy
// workgroup in two steps.  texel_put, by the thread of a pixel inside the image: {nx, ny, nz, depth}, copies of the normal's xyz
// and of the depth image's own value d.  texel_block_max, by every thread, with pixel_xy's lane and wave and that d, or -inf for a
// thread without a pixel:
// the maximum finite depth of each 8 x 4 block of the workgroup's 64 x 4 pixels (-inf where a block has none; fmaxf drops NaN),
// in rows of bw8 floats, one row per four image rows.  s_max: PIX_H x 8 floats of LDS; a barrier inside.
__device__ __forceinline__ void texel_put(unsigned char* tex, size_t tpitch, int u, int v, float4 N, float d)
{
    reinterpret_cast<float4*>(tex + (size_t)v * tpitch)[u] = make_float4(N.x, N.y, N.z, d);
}
__device__ __forceinline__ void texel_block_max(float* bmax, unsigned bw8, int lane, int wv, float d, float (*s_max)[8])
{
    static_assert(PIX_W == 64 && PIX_H == 4, "eight 8-lane blocks per wave, four waves");
    d = wave8_combine(fmaxf(d, -__builtin_inff()), FMax{});
    if ((lane & 7) == 0) s_max[wv][lane >> 3] = d;
    __syncthreads();
    if (threadIdx.x < 8)
        bmax[(size_t)blockIdx.y * bw8 + blockIdx.x * 8 + threadIdx.x] =
            fmaxf(fmaxf(s_max[0][threadIdx.x], s_max[1][threadIdx.x]), fmaxf(s_max[2][threadIdx.x], s_max[3][threadIdx.x]));
}

// The tracked SdfFuse's kept set (fuse.hip, fuse_launch): y-brick row `row` of the parent volume belongs to it
__host__ __device__ inline bool keep_row(int row, int stride) { return stride > 0 && (unsigned)row % (unsigned)stride == 0u; }

} // namespace kfx

// ---- brick summary of a TSDF volume (kfx_sdf_summary, include/kfx.h; summary.hip) -----------------------------------
// R: one float4 {lo, hi, state, -} per 8 x 8 x 8 cells, kept current by the TRACK fuse kernels (state 0: every cell holds
// a value in [lo, hi]; 1: every cell is NaN; 2: every cell is NaN or holds a value in [lo, hi] -- an invalidated brick has
// the infinite range).  C: what the ray-march reads (ClassView below), built from R on demand.
// (KFX_SUMMARY_RING and the layout of a ring slot: summary_ring_host.h)
struct kfx_sdf_summary {
    float4* R;
    int nbx, nby, nbz;
    int w, h, d;                 // parent volume (cells)
    int cell_bytes;              // 8: SDF_t cells (kfx_sdf_summary_create), 4: SDF_h cells (kfx_sdf_summary_create_h)
    const unsigned char* base;   // parent volume storage
    size_t pitch, img_pitch;
    // class tables of the march (ClassView below): two bit planes per entry, fine level (8^3 or 16^3 cells) then 32^3 cells
    unsigned* C;                 // device, sized for the finest level
    int c_dirty;                 // R changed since C was built: 0 no; 1 maybe (a tracked SdfFuse ran: the device word d_dirty knows); 2 yes
    float c_lo_ok, c_hi_ok;      // the band of (c_tol, c_vref): what the tracked SdfFuse compares brick masks with (brick_class_mask)
    float c_tol, c_vref;         // what C was built with
    int c_shift;                 // fine level C was built for (log2 of its cells per entry)
    int c_global;                // C also holds the 64^3- and 128^3-cell levels (the global-table mode, raycast.hip class_view)
    int n_coarse;                // 32^3-cell entries
    // device: {running count of 32^3-cell entries of class != 0, workgroups of the build's counting launch that have arrived
    // (all of them, those of the fine level included, where one launch builds both levels), the count of the last real build,
    // conditional builds that built, conditional builds that returned early -- one increment of either per conditional build}
    int* d_count;
    // device word: some brick's class mask (brick_class_mask) changed since C was built.  Set by the tracked SdfFuse kernels,
    // read by every workgroup of a conditional table build (summary.hip) before anything else, cleared by the last one to arrive.
    int* d_dirty;
    // The table builds publish their count of 32^3-cell entries of class != 0 in a host-visible ring (pinned, mapped) of 64-bit
    // slots {stamp of the build, count} (summary_ring_host.h): build b writes slot b % KFX_SUMMARY_RING with one system-scope
    // store, nothing is recorded behind it.  The tracked raycast chooses its kernel from the count of build b - 2 (raycast.hip,
    // class_view): old enough to have finished without anybody waiting -- the slot carries that build's stamp by then, and the
    // reader looks until it does -- and, unlike "whatever the last finished build said", the same choice for the same sequence of calls.
    unsigned long long* h_skippable;   // the ring, host address (nullptr: no pinned memory; the tables are always used)
    unsigned long long* d_skippable;   // the ring, device address
    unsigned builds;             // table builds issued so far
    unsigned long long launches; // kernel launches summary_classes_prepare has issued so far (kfx_debug_summary_top_levels)
    unsigned plain_calls;        // tracked raycasts since the choice last fell on the plain march (the tables are then rebuilt every 8th call only)
    unsigned sweeps;             // tracked SdfFuse launches so far: every other one walks the planes from the far end (fuse.hip)
    // the kept set of the last tracked SdfFuse launch (fuse.hip, fuse_launch; read by kfx_debug_fuse_keep): the y-brick rows
    // [keep_row0, keep_row0 + keep_rows) of the parent volume it covered, those with keep_row(row, keep_stride) read with ordinary loads
    int keep_stride, keep_row0, keep_rows;
};
namespace kfx {
// The class tables the march stages in LDS.  Per entry (a cube of 2^shift cells, together with the +1 cells a trilinear sample
// based in it reads) two bits: 0 = sample; 1 = every cell holds vref (exact numerics: that bit pattern; fast numerics: within
// tol) -- a sample there IS vref; 2 = every cell is NaN; 3 = every cell is NaN or holds vref -- the reference's step from
// there is trunc either way (a NaN sample steps by trunc, cu_raycast.cu:77-80, and vref = trunc >= min_delta), only
// last_sdf is undecided, and the march settles it with one sample if the next one is a crossing.  A row of entries along x
// is stored as uint2 {plane 0, plane 1} per 32 entries.
struct ClassLevel {
    int shift;        // log2(cells per entry along an axis)
    int ny;           // entries along y
    int rw;           // 32-bit words per row of entries: 2 * ceil(nx / 32)
    int first;        // first word of the level in the table
};
struct ClassView {
    const unsigned* C;   // global copy (fine level, then the 32^3 level)
    ClassLevel fine, coarse;
    int words;           // total 32-bit words
    float vref;          // the value of class 1 (= the launch's trunc_dist)
    float tol;           // relative tolerance the tables were built with (0: exact numerics)
    int amb_ok;          // class 3 may be skipped (trunc >= min_delta)
    int ox, oy, oz;      // cell offset of the view inside the parent volume
    float eps;           // margin (cells) that covers the error of the affine cell estimate
    // Coarser levels (64^3 and 128^3 cells; an entry = the combination of its 2 x 2 x 2 children, which include their +1 cells):
    // the last workgroup of a table build derives them from the 32^3-cell level into the words behind it (classes_level_up), and
    // the raycast workgroups stage them with the rest.  nx5 / nz5: entries of the 32^3-cell level along x / z (ny5 = coarse.ny);
    // top_n: how many coarser levels the march consults (0-2); lds_words: the words a workgroup stages.
    int nx5, nz5, top_n, lds_words;
    // Global-table mode (class tables larger than the LDS budget, or KFX_RAYCAST_GLOBAL_TABLES=1): the table build also writes the
    // 64^3- and 128^3-cell levels to global memory behind the 32^3-cell level (top_first); a workgroup stages only those two
    // (lds_words from word top_first) and looks the fine and 32^3-cell levels up in global memory, coarse level first.
    // LDS mode: the staged words are [0, words).
    int global, top_first;
};
// What the class of an entry depends on a brick through: bit 0 every cell NaN, bit 1 every cell holds vref (within the band),
// bit 2 every cell is NaN or holds vref.  The table builds (class_row, summary.hip) combine these, and the tracked SdfFuse
// compares a brick's mask before and after its update: while no mask changes, the tables stay what they are.
__device__ __forceinline__ unsigned brick_class_mask(const float lo, const float hi, const int state, const float lo_ok, const float hi_ok)
{
    const bool in_band = lo >= lo_ok && hi <= hi_ok;   // every valued cell of the brick holds vref (false for the unknown state's infinite range)
    return (state == 1 ? 1u : 0u) | ((state == 0 && in_band) ? 2u : 0u) | ((state == 1 || in_band) ? 4u : 0u);
}
// geometry of a level derived from a finer one with nx x ny x nz entries, placed at word `first`
inline __host__ __device__ void class_level_up(const int nx, const int ny, const int nz, const int shift, const int first, ClassLevel& L, int& ux, int& uz, int& words)
{
    ux = (nx + 1) >> 1; uz = (nz + 1) >> 1;
    L.shift = shift; L.ny = (ny + 1) >> 1; L.rw = 2 * ((ux + 31) >> 5); L.first = first;
    words = (L.rw * L.ny * uz + 3) & ~3;
}
// one derived level: entry (bx, by, bz) = combination of the 2 x 2 x 2 entries of `src` below it (edge entries repeat a
// neighbour: same verdict).  One entry per thread and round: rows are padded to a power of two (or to whole waves when they are
// longer than a wave), so a wave's 64 lanes hold whole rows side by side, the two bit planes are its ballots, and the first
// lane of each row writes the row's share of them.
__device__ __forceinline__ void classes_level_up(unsigned* tab, const ClassLevel& src, int snx, int snz, const ClassLevel& dst, int dnx, int dnz)
{
    const int lane = threadIdx.x & 63;
    int lg = 0;                                      // log2 of the padded row length, at most 6 ...
    while ((1 << lg) < dnx && lg < 6) ++lg;
    const int chunks = (dnx + 63) >> 6;              // ... rows longer than a wave take `chunks` waves
    const int px = chunks > 1 ? chunks << 6 : 1 << lg;
    const int total = px * dst.ny * dnz;
    for (int e0 = 0; e0 < total; e0 += 256) {        // uniform: every wave runs the same number of rounds (ballots below)
        const int e = e0 + (int)threadIdx.x;
        const int bx = chunks > 1 ? e % px : e & (px - 1), r = chunks > 1 ? e / px : e >> lg;
        const int by = r % dst.ny, bz = r / dst.ny;
        int cls = 0;
        if (e < total && bx < dnx) {
            bool all_free = true, all_nan = true, all_either = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int x = min(2 * bx + (k & 1), snx - 1), y = min(2 * by + ((k >> 1) & 1), src.ny - 1), z = min(2 * bz + (k >> 2), snz - 1);
                const uint2 w = *reinterpret_cast<const uint2*>(tab + src.first + (z * src.ny + y) * src.rw + ((x >> 5) << 1));
                const int c = (int)((w.x >> (x & 31)) & 1u) | (int)(((w.y >> (x & 31)) & 1u) << 1);
                all_free = all_free && c == 1;
                all_nan = all_nan && c == 2;
                all_either = all_either && c != 0;
            }
            cls = all_free ? 1 : (all_nan ? 2 : (all_either ? 3 : 0));
        }
        const unsigned long long p0 = __ballot(cls & 1), p1 = __ballot(cls & 2);
        if (e < total && (bx & 63) == 0 && (chunks > 1 || bx == 0)) {   // first lane of a row (or of a row's 64-entry chunk)
            const int sh = chunks > 1 ? 0 : lane;                        // where the row's bits start in the ballots
            const unsigned long long m = (chunks > 1 || lg == 6) ? ~0ull : ((1ull << (1 << lg)) - 1ull);
            const unsigned long long r0 = (p0 >> sh) & m, r1 = (p1 >> sh) & m;
            unsigned* out = tab + dst.first + (bz * dst.ny + by) * dst.rw + (bx >> 6) * 4;
            out[0] = (unsigned)r0; out[1] = (unsigned)r1;
            if ((bx >> 6) * 4 + 2 < dst.rw) { out[2] = (unsigned)(r0 >> 32); out[3] = (unsigned)(r1 >> 32); }
        }
    }
}
// global = 1: also build the 64^3- and 128^3-cell levels in global memory (at word summary_top_first)
int summary_classes_prepare(kfx_sdf_summary* s, float tol, float vref, int fine_shift, hipStream_t stream, int global = 0);
void summary_class_layout(const kfx_sdf_summary* s, int fine_shift, ClassView& cv);
// words of the table with the two derived levels behind the 32^3-cell level: first word of the 64^3 level, the two levels' words
void summary_top_layout(const ClassView& cv, ClassLevel& l6, ClassLevel& l7, int& w6, int& w7);
// cell offset of a view of the summary's parent volume (same pitches, pointer inside the parent): 0 on success
int summary_view_offset(const kfx_sdf_summary* s, const kfx_volume* view, int* ox, int* oy, int* oz);
} // namespace kfx

// ---- host-side launch helpers (capi.hip) --------------------------------------
namespace kfx {
int set_error(int code, const char* what);
int check_launch(const char* what);
int hip_status(hipError_t e, const char* what);   // 0, or the error cleared and reported as `what`
int math_mode(); // KFX_MATH_EXACT / KFX_MATH_FAST
// kfx_frame_step's pair (frame.hip): the fused vbo / normals launch also writes the packed texel image {nx, ny, nz, depth} that the
// SdfFuse of the same frame stages by LDS-DMA (preprocess.hip, fuse.hip; host_args.h: tex_layout); texels may be null
int depth_to_vbo_normals_texels(const kfx_image* vbo, const kfx_image* nrm, const kfx_image* depth, const float K[4], float scale,
                                const kfx_image* texels, kfx_stream stream);
int sdf_fuse_slab_texels(const kfx_volume* vol, const kfx_slab* slab, const kfx_image* depth, const kfx_image* norm, const kfx_image* texels,
                         const float T_cw[12], const float K[4], float trunc_dist, float max_w, float mincostheta, unsigned flags, kfx_stream stream);
int sdf_fuse_texels(const kfx_volume* vol, kfx_sdf_summary* summary, const kfx_image* depth, const kfx_image* norm, const kfx_image* texels,
                    const float T_cw[12], const float K[4], float trunc_dist, float max_w, float mincostheta, unsigned flags, kfx_stream stream);
} // namespace kfx
