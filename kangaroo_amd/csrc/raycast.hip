// raycast.hip -- per-pixel sphere-traced ray-march of the TSDF (roo::RaycastSdf) for gfx950.
//
// Reference behaviour: src/cu_raycast.cu:14-113 (PhongShade, KernRaycastSdf) with the
// samplers of BoundedVolume.h:93-106 / Volume.h:224-295.  New kernel: a wave64 owns a
// 32x2 pixel tile (coherent rays: the kernel is bound by the number of distinct 64-byte lines a
// wave touches per step, and cells are contiguous along x -- 8x8 tiles were 18 % slower, A/B in
// scripts/raycast_ab.py), a workgroup is 2x2 such tiles; each trilinear sample is four 16-byte
// loads (the x and x+1 cells of an AoS row are contiguous) instead of eight 8-byte ones;
// the gradient stencil is 20 distinct cells instead of 32 loads; missed rays skip the
// (discarded) normal evaluation of the reference.
#include <cmath>
#include <thread>

#include <hip/hip_fp16.h>

#include "kfx_device.h"
#include "sampling.h"
#include "raycast_ray.h"
#include "../../include/kfx_slab_color.h"

namespace kfx {

// write_ray (raycast_ray.h) on a dense volume: the gradient from its pitched rows; COLOR: the colour volume's sample for the shade
template <typename CELL, bool COLOR>
__device__ __forceinline__ void write_ray(const RayParams& q, const ColorGeom& cv, const int u, const int v, const float depth)
{
    const auto gradient_at = [&q](const V3 pos_w) { return gradient<CELL>(q, pos_w); };
    if constexpr (COLOR) write_ray(q, u, v, depth, gradient_at, [&cv](const V3 pos_w) { return trilinear<RayC32>(cv, pos_w); });
    else write_ray(q, u, v, depth, gradient_at, PhongShade{});
}

// COUNT mode of the marches (kfx_raycast_sdf_count[_tracked]): every cell a sample or a hit's gradient stencil reads is marked
// in a bitmap (one bit per voxel, dense x-fastest index) and counted in cnt[] = {samples, table look-ups, hits, newly marked
// cells}; no image is written.  U = distinct voxels touched is the figure SURVEY.md 8(d) prices RaycastSdf's algorithmic bytes
// with (8 B x U + 24 B x w h).
__device__ __forceinline__ unsigned touch(unsigned* bitmap, const VolView& v, int x, int y, int z)
{
    const size_t i = ((size_t)z * v.h + y) * v.w + x;
    const unsigned bit = 1u << (i & 31);
    unsigned* word = bitmap + (i >> 5);
    if (*reinterpret_cast<volatile unsigned*>(word) & bit) return 0u;
    return (atomicOr(word, bit) & bit) ? 0u : 1u;
}
// one sample: its 8 cells (c by value: behind a reference touch()'s atomics make the compiler reload it, at the price of SGPR spills)
__device__ __forceinline__ void touch_sample(unsigned* bitmap, const VolView& vol, const CellPos c, unsigned* cnt)
{
    cnt[0] += 1;
    for (int k = 0; k < 8; ++k) cnt[3] += touch(bitmap, vol, c.ix + (k & 1), c.iy + ((k >> 1) & 1), c.iz + (k >> 2));
}
// one hit: the gradient's 20 cells, {-1, 0, 1}^3 around its base cell with at most one coordinate at -1 (sampling.h)
__device__ __forceinline__ void touch_gradient(unsigned* bitmap, const RayParams& p, const V3 pos_w, unsigned* cnt)
{
    cnt[2] += 1;
    const CellPos b = gradient_base(p, pos_w);
    for (int dz = -1; dz < 2; ++dz)
        for (int dy = -1; dy < 2; ++dy)
            for (int dx = -1; dx < 2; ++dx)
                if ((dx < 0) + (dy < 0) + (dz < 0) <= 1) cnt[3] += touch(bitmap, p.vol, b.ix + dx, b.iy + dy, b.iz + dz);
}
// a wave's counts into counters[] = {samples, rays that enter the box, hits, U, table look-ups} (include/kfx_debug.h)
__device__ __forceinline__ void publish_counts(const unsigned* cnt, const unsigned entered, unsigned long long* counters)
{
    unsigned c[5] = {cnt[0], entered, cnt[2], cnt[3], cnt[1]};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int k = 0; k < 5; ++k) c[k] += __shfl_xor(c[k], off, 64);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (c[k]) atomicAdd(&counters[k], (unsigned long long)c[k]);
    }
}

// one ray: KernRaycastSdf (cu_raycast.cu:34-113) for pixel (u, v).  Returns the value written to the depth image.
template <typename CELL, bool COLOR, bool COUNT = false>
__device__ __forceinline__ float raycast_pixel(const RayParams& p, const ColorGeom& cv, const int u, const int v, unsigned* bitmap = nullptr,
                                               unsigned* cnt = nullptr)
{
    if (u >= p.w || v >= p.h) return 0.f;

    const RayBox box = ray_box(p, u, v);
    float depth = 0.0f;
    if (enters(box))
        depth = march_plain(p, box, [=](const RayParams& q, const V3 pos_w) {
            if constexpr (COUNT) touch_sample(bitmap, q.vol, cell_of(q, pos_w), cnt);
            return trilinear<CELL>(q, pos_w);
        });

    if constexpr (COUNT) {
        if (depth > 0) touch_gradient(bitmap, p, box.c_w + box.ray_w * depth, cnt);
    } else {
        write_ray<CELL, COLOR>(p, cv, u, v, depth);
    }
    return depth > 0 ? depth : __builtin_nanf("");
}

// ---------------------------------------------------------------------------------------
// The march through the class tables (ClassView, kfx_device.h).  Every workgroup stages the tables -- a
// 32^3-cell level and a finer one, two bits per entry -- in LDS.  In an iteration a ray does ONE of two things:
//   * it consults the tables (LDS and arithmetic only): if the entry of its position says what a sample there would be --
//     trunc, NaN, or "trunc or NaN" -- the reference's step is known, and with it every following step that still starts
//     inside the entry: the whole run is taken at once (exact numerics: the reference's own lambda += delta additions, one
//     per step; fast numerics: one multiply-add);
//   * or it samples, exactly as the plain kernel does.
// The sampling lanes of a wave request their cells first and the consulting lanes work while those loads are in flight.
// The entry of a position comes from an affine estimate of the base-cell coordinate, pf(lambda) = A + B lambda: three FMAs
// instead of the ~30 separately rounded operations of cell_of().  The estimate is within `eps` cells of cell_of()'s
// coordinate (bound evaluated on the host from the box, the camera and the roundings of both, class_view()), a position
// closer than eps to a cell boundary -- where the two could disagree about the base cell -- is sampled, with cell_of()
// itself, and runs end eps inside the entry: the skipped steps are exactly those of the reference march, so with the
// exact-numerics tables (tol = 0: cells bit-equal to trunc, or NaN) depth, normals and shade stay bit-identical to the
// plain march.
// ---------------------------------------------------------------------------------------
// The coarser levels of the workgroup (ClassView::top_n of them: 64^3 and 128^3 cells, staged behind the others by classes_stage), described
// where the march can read them without holding them in registers across its loop.
struct TopLevels { ClassLevel lv[2]; int n; };

__device__ __forceinline__ int class_lookup(const unsigned* tab, const ClassLevel& L, int gx, int gy, int gz)
{
    const int bx = gx >> L.shift, by = gy >> L.shift, bz = gz >> L.shift;
    const uint2 w = *reinterpret_cast<const uint2*>(tab + L.first + (bz * L.ny + by) * L.rw + ((bx >> 5) << 1));
    return (int)((w.x >> (bx & 31)) & 1u) | (int)(((w.y >> (bx & 31)) & 1u) << 1);
}

// GT (global-table mode, ClassView::global): the fine and 32^3-cell levels are read from global memory (cl.C), the 64^3 and
// 128^3 levels from LDS, and the levels are consulted coarse-first: a coarse entry of class != 0 implies that every entry below
// it is != 0, so the coarsest level with class != 0 is the one the fine-first order of the LDS mode arrives at -- the same
// runs, the same images -- and a ray in wide free space does not touch the global tables.
// COUNT: as raycast_pixel's.
template <typename CELL, bool COLOR, bool COUNT = false, bool GT = false>
__device__ __forceinline__ float raycast_pixel_classes(const RayParams& p, const RayParams& q, const ColorGeom& cv, const int u, const int v, const ClassView& cl_arg, const unsigned* tab,
                                                       const TopLevels& top, unsigned* bitmap = nullptr, unsigned* cnt = nullptr)
{
    // The loop's uniforms fill the scalar register file, and what does not fit comes back with a v_readlane on the march's chain
    // of dependent instructions.  So: p are the launch parameters as kernel arguments (scalar registers), q the workgroup's copy of
    // them in LDS, which the epilogue reads -- pose, intrinsics, output images and the gradient's geometry are not held across the
    // march; and (LDS mode) the table descriptors and the view's offsets and margins are parked in vector registers (in_vgpr,
    // kfx_device.h; VGPRs are not this kernel's limit) -- the same values in the same expressions.
    constexpr bool PARK = !GT && !COUNT;
    ClassView parked;
    if constexpr (PARK) parked = cl_arg;
    ClassView& clp = parked;
    if constexpr (PARK) {
        clp.fine.shift = in_vgpr(clp.fine.shift); clp.fine.ny = in_vgpr(clp.fine.ny); clp.fine.rw = in_vgpr(clp.fine.rw); clp.fine.first = in_vgpr(clp.fine.first);
        clp.coarse.ny = in_vgpr(clp.coarse.ny); clp.coarse.rw = in_vgpr(clp.coarse.rw); clp.coarse.first = in_vgpr(clp.coarse.first);
        clp.ox = in_vgpr(clp.ox); clp.oy = in_vgpr(clp.oy); clp.oz = in_vgpr(clp.oz);
        clp.eps = in_vgpr(clp.eps); clp.vref = in_vgpr(clp.vref);
    }
    const ClassView& cl = PARK ? parked : cl_arg;
    if (u >= p.w || v >= p.h) return 0.f;

    const RayBox box = ray_box(p, u, v);
    const V3 c_w = box.c_w, ray_w = box.ray_w;
    const float max_tmin = box.max_tmin, min_tmax = box.min_tmax;

    float depth = 0.0f;
    if (max_tmin < min_tmax) {
        float lambda = max_tmin;
        float last_sdf = __builtin_nanf("");
        const float min_delta = p.voxel.x;
        float delta = 0.f;
        // base-cell coordinate along the ray (an estimate: see above), and what leaving an entry costs per axis
        const V3 sc = v3(p.dims1.x / p.size.x, p.dims1.y / p.size.y, p.dims1.z / p.size.z);
        const V3 pfA = v3((c_w.x - p.vol.bmin.x) * sc.x, (c_w.y - p.vol.bmin.y) * sc.y, (c_w.z - p.vol.bmin.z) * sc.z);
        const V3 pfB = v3(ray_w.x * sc.x, ray_w.y * sc.y, ray_w.z * sc.z);
        const V3 inv = v3(1.0f / pfB.x, 1.0f / pfB.y, 1.0f / pfB.z);   // +-inf for a ray parallel to an axis plane: that axis never ends a run
        const float eps = cl.eps;
        const float step_free = fmaxf(cl.vref, min_delta);               // the reference's delta for sdf = vref
        const float inv_step_free = 1.0f / step_free, inv_trunc = 1.0f / p.trunc;
        const float band = cl.tol * cl.vref;
        bool pending = false;      // last_sdf is "vref or NaN": the last step left an entry of class 3
        float lambda_prev = 0.f;   // where that step started
        // The tables are consulted where they can help: at the start, after a run, and after a sample that came back as vref
        // or NaN (free or unseen space); a sample with any other value lies in an entry of class 0.  After a class-0 answer the
        // ray first leaves that entry (lam_retry).  A ray through a band of mixed values therefore marches as the plain kernel.
        bool consult = true;
        float lam_retry = lambda;
        int wait = 0, backoff = 1;   // samples to let pass before the next look at the tables: doubles with every class-0 answer
        // One iteration of a wave: the lanes that sample request their cells; the lanes that consult the tables do so (LDS and
        // arithmetic only) while those loads are in flight; then the sampling lanes wait, blend and step.  A lane whose
        // entry turns out to be class 0 samples in the next iteration.
        while (lambda < min_tmax) {
            const bool look = consult && wait == 0 && lambda >= lam_retry;
            CellPos c{};
            typename CELL::InFlight fl;
            if (!look) {
                c = cell_of(p, c_w + ray_w * lambda);
                trilinear_issue<CELL>(fl, p, c);
                if constexpr (COUNT) touch_sample(bitmap, p.vol, c, cnt);
            }
            if (look) {
                if constexpr (COUNT) cnt[1] += 1;
                const float ex = __builtin_fmaf(pfB.x, lambda, pfA.x), ey = __builtin_fmaf(pfB.y, lambda, pfA.y), ez = __builtin_fmaf(pfB.z, lambda, pfA.z);
                const float flx = floorf(ex), fly = floorf(ey), flz = floorf(ez);
                const float lo_f = fminf(fminf(ex - flx, ey - fly), ez - flz), hi_f = fmaxf(fmaxf(ex - flx, ey - fly), ez - flz);
                // inside [0, dims - 1) with the margin on every axis: the base cell is floor(pf), no clamp involved; and at least
                // eps away from every cell boundary: cell_of() finds the same base cell
                bool run = false;
                if (fminf(fminf(ex, ey), ez) > eps && ex < p.dims1.x - eps && ey < p.dims1.y - eps && ez < p.dims1.z - eps && lo_f > eps && hi_f < 1.0f - eps) {
                    const int gx = (int)flx + cl.ox, gy = (int)fly + cl.oy, gz = (int)flz + cl.oz;
                    int cls = 0, shift = cl.fine.shift;
                    if constexpr (GT) {
                        // coarse-first: 128^3 and 64^3 cells (LDS), then 32^3 cells and the fine level (global, uint2 loads)
                        if (cl.top_n > 1) {
                            int c7 = class_lookup(tab, top.lv[1], gx, gy, gz);
                            if (c7 == 3 && !cl.amb_ok) c7 = 0;
                            if (c7 != 0) { cls = c7; shift = 7; }
                        }
                        if (cls == 0 && cl.top_n > 0) {
                            int c6 = class_lookup(tab, top.lv[0], gx, gy, gz);
                            if (c6 == 3 && !cl.amb_ok) c6 = 0;
                            if (c6 != 0) { cls = c6; shift = 6; }
                        }
                        if (cls == 0) {
                            int c5 = class_lookup(cl.C, cl.coarse, gx, gy, gz);
                            if (c5 == 3 && !cl.amb_ok) c5 = 0;
                            if (c5 != 0) { cls = c5; shift = 5; }
                        }
                        if (cls == 0) {
                            cls = class_lookup(cl.C, cl.fine, gx, gy, gz);
                            if (cls == 3 && !cl.amb_ok) cls = 0;
                            shift = cl.fine.shift;
                        }
                    } else {
                    // the fine level answers "sample here?"; only a positive answer is worth the second look that may extend
                    // the run to the whole 32^3-cell entry
                    cls = class_lookup(tab, cl.fine, gx, gy, gz);
                    if (cls == 3 && !cl.amb_ok) cls = 0;
                    if (cls != 0 && cl.fine.shift < 5) {
                        int c5 = class_lookup(tab, cl.coarse, gx, gy, gz);
                        if (c5 == 3 && !cl.amb_ok) c5 = 0;
                        if (c5 != 0) { cls = c5; shift = 5; }
                    }
                    // ... and a run through 32^3 cells may be one through 64^3 or 128^3 (the levels the table build derived from it):
                    // wide free or never-observed space is crossed in a third of the look-ups
                    if (shift == 5 && cl.top_n > 0) {
                        int c6 = class_lookup(tab, top.lv[0], gx, gy, gz);
                        if (c6 == 3 && !cl.amb_ok) c6 = 0;
                        if (c6 != 0) {
                            cls = c6; shift = 6;
                            if (cl.top_n > 1) {
                                int c7 = class_lookup(tab, top.lv[1], gx, gy, gz);
                                if (c7 == 3 && !cl.amb_ok) c7 = 0;
                                if (c7 != 0) { cls = c7; shift = 7; }
                            }
                        }
                    }
                    }
                    // the entry's cells are [lo, lo + L) per axis in the view's coordinates; its far side along the ray, pulled in
                    // by the margin: positions up to there certainly have their base cell in the entry
                    const float L = (float)(1 << shift);
                    const float lox = (float)(((gx >> shift) << shift) - cl.ox), loy = (float)(((gy >> shift) << shift) - cl.oy),
                                loz = (float)(((gz >> shift) << shift) - cl.oz);
                    const float bx = pfB.x >= 0.f ? lox + L - eps : lox + eps, by = pfB.y >= 0.f ? loy + L - eps : loy + eps,
                                bz = pfB.z >= 0.f ? loz + L - eps : loz + eps;
                    const float lam_exit = fminf(fminf((bx - pfA.x) * inv.x, (by - pfA.y) * inv.y), (bz - pfA.z) * inv.z);
                    if (cls != 0) {
                        // the reference's step for a sample of vref (class 1) or NaN (2; 3: the two steps are equal), taken from
                        // this position and from the following ones that still start inside the entry (and the box): n steps,
                        // n - 1 <= (lam_last - lambda) / delta less a hundredth for the quotient's rounding
                        delta = cls == 1 ? step_free : p.trunc;
                        // (half cells, fast numerics: the band is wide enough to take cells just inside the truncation band in
                        // front of a surface, so a crossing right after a class-1 run settles last_sdf with one sample too)
                        pending = cls == 3 || (CELL::BYTES == 4 && cls == 1 && cl.tol > 0.f);
                        last_sdf = cls == 1 ? cl.vref : __builtin_nanf("");
                        const float lam_last = fminf(lam_exit, min_tmax);
                        const float more = fminf(floorf((lam_last - lambda) * (cls == 1 ? inv_step_free : inv_trunc) - 0.01f), 4096.f);
                        if (cl.tol > 0.f) {
                            // fast numerics: the run in one multiply-add (the sum differs from n separately rounded additions by a
                            // few ulp of lambda: far inside the mode's tolerance)
                            const float nm = fmaxf(more, 0.f);
                            lambda_prev = __builtin_fmaf(nm, delta, lambda);
                            lambda = lambda_prev + delta;
                        } else {
                            // exact numerics: the reference's own additions, one per step
                            lambda_prev = lambda;
                            lambda += delta;
                            for (int k = (int)more; k > 0; --k) { lambda_prev = lambda; lambda += delta; }
                        }
                        backoff = 1;
                        run = true;
                    } else {
                        lam_retry = lam_exit;   // class 0: nothing to learn before the ray has left this entry
                    }
                }
                if (!run) {
                    wait = backoff;
                    backoff = min(backoff * 2, 32);
                }
            }
            if (!look) {
                const float sdf = trilinear_finish<CELL>(fl, c);
                wait = max(wait - 1, 0);
                if (sdf <= 0) {
                    // a crossing needs the previous sample's value: the one thing a class-3 step left open
                    if (pending) {
                        last_sdf = trilinear<CELL>(p, c_w + ray_w * lambda_prev);
                        if constexpr (COUNT) touch_sample(bitmap, p.vol, cell_of(p, c_w + ray_w * lambda_prev), cnt);
                    }
                    if (last_sdf > 0) {
                        if (p.subpix) lambda = lambda + delta * sdf / (last_sdf - sdf);
                        depth = lambda;
                    }
                    break;
                }
                delta = march_step(sdf, min_delta, p.trunc);
                lambda += delta;
                last_sdf = sdf;
                pending = false;
                consult = !(fabsf(sdf - cl.vref) > band);   // vref (within the tables' tolerance) or NaN
            }
        }
    }

    if constexpr (COUNT) {
        if (depth > 0) touch_gradient(bitmap, p, c_w + ray_w * depth, cnt);
    } else {
        write_ray<CELL, COLOR>(q, cv, u, v, depth);
    }
    return depth > 0 ? depth : __builtin_nanf("");
}

// workgroup prologue of the class-table kernels: the tables into LDS (16-byte loads, all in flight together) -- the fine and the
// 32^3-cell level and, behind them, as many of the 64^3- and 128^3-cell levels as the march consults (cl.top_n): the table
// build derived those once (classes_count_and_top, summary.hip), nothing is derived here
// (GT: only the 64^3- and 128^3-cell levels, staged at word 0)
template <bool GT = false>
__device__ __forceinline__ void classes_stage(const ClassView& cl, unsigned* tab, TopLevels& top)
{
    const uint4* src = reinterpret_cast<const uint4*>(cl.C + (GT ? cl.top_first : 0));
    uint4* dst = reinterpret_cast<uint4*>(tab);
    for (int i = threadIdx.x; i < (cl.lds_words >> 2); i += blockDim.x) dst[i] = src[i];
    ClassLevel l6, l7;
    int nx6, nz6, nx7, nz7, w6, w7;
    const int at = GT ? 0 : cl.words;
    class_level_up(cl.nx5, cl.coarse.ny, cl.nz5, 6, at, l6, nx6, nz6, w6);
    class_level_up(nx6, l6.ny, nz6, 7, at + w6, l7, nx7, nz7, w7);
    if (threadIdx.x == 0) { top.lv[0] = l6; top.lv[1] = l7; top.n = cl.top_n; }
    __syncthreads();
}

// does any thread of the workgroup say yes?  One barrier: a ballot per wave, the verdicts of the four waves of a 256-thread
// workgroup (every kernel that calls this has __launch_bounds__(256) and is launched with dim3(256)) through LDS.
__device__ __forceinline__ bool workgroup_any(const bool yes, int* s_any)
{
    const bool wave_any = __ballot(yes) != 0ull;
    if ((threadIdx.x & 63) == 0) s_any[threadIdx.x >> 6] = wave_any ? 1 : 0;
    __syncthreads();
    return (s_any[0] | s_any[1] | s_any[2] | s_any[3]) != 0;
}

template <typename CELL, bool GT = false>
__global__ __launch_bounds__(256) void k_raycast_sdf_classes(const RayParams p, const ClassView cl)
{
    extern __shared__ unsigned s_tab[];
    __shared__ RayParams s_p;
    __shared__ TopLevels s_top;
    __shared__ int s_any[4];   // (workgroup_any: one word per wave of the 256-thread workgroup)
    if (threadIdx.x == 0) s_p = p;
    int u, v;
    const bool carries = ray_lane_pixel(p, p.sparse_lanes, blockIdx.x, blockIdx.y, u, v);
    // a workgroup without a ray in the box (S_full at 640 x 480: seven in ten) writes "no hit" and leaves before the prologue
    const bool pixel = carries && u < p.w && v < p.h;
    // (LDS mode; the global-table kernel's register allocation does not take the extra live ranges)
    if constexpr (!GT) {
        if (!workgroup_any(pixel && enters(ray_box(p, u, v)), s_any)) {   // (every thread arrives: idle lanes leave after it)
            if (pixel) write_no_hit(ray_out(p, u, v));
            return;
        }
    }
    classes_stage<GT>(cl, s_tab, s_top);   // (barrier inside)
    if (!carries) return;
    raycast_pixel_classes<CELL, false, false, GT>(p, s_p, ColorGeom{}, u, v, cl, s_tab, s_top);
}

template <typename CELL, bool COLOR>
__global__ __launch_bounds__(256) void k_raycast_sdf(const RayParams p, const ColorGeom cv)
{
    int u, v;
    if (!ray_lane_pixel(p, p.sparse_lanes, blockIdx.x, blockIdx.y, u, v)) return;
    raycast_pixel<CELL, COLOR>(p, cv, u, v);
}

// Diagnostics (kfx_raycast_sdf_count): the march of k_raycast_sdf in COUNT mode.  counters: {samples, rays that enter the box, hits, U}.
template <typename CELL>
__global__ __launch_bounds__(256) void k_raycast_sdf_count(const RayParams p, unsigned* __restrict__ bitmap, unsigned long long* __restrict__ counters)
{
    int u, v;
    ray_pixel_of(p, blockIdx.x, blockIdx.y, threadIdx.x, u, v);
    unsigned cnt[4] = {0u, 0u, 0u, 0u}, entered = 0;
    if (u < p.w && v < p.h) {
        entered = enters(ray_box(p, u, v)) ? 1u : 0u;
        raycast_pixel<CELL, false, true>(p, ColorGeom{}, u, v, bitmap, cnt);
    }
    publish_counts(cnt, entered, counters);
}

// the same for the march through the class tables: counters = {samples, rays that enter the box, hits, U, table look-ups, table bytes}
template <typename CELL, bool GT = false>
__global__ __launch_bounds__(256) void k_raycast_sdf_classes_count(const RayParams p, const ClassView cl, unsigned* __restrict__ bitmap,
                                                                   unsigned long long* __restrict__ counters)
{
    extern __shared__ unsigned s_tab[];
    __shared__ RayParams s_p;
    __shared__ TopLevels s_top;
    if (threadIdx.x == 0) s_p = p;
    classes_stage<GT>(cl, s_tab, s_top);   // (barriers inside)
    int u, v;
    ray_pixel_of(p, blockIdx.x, blockIdx.y, threadIdx.x, u, v);
    unsigned cnt[4] = {0u, 0u, 0u, 0u}, entered = 0;
    if (u < p.w && v < p.h) {
        entered = enters(ray_box(p, u, v)) ? 1u : 0u;
        raycast_pixel_classes<CELL, false, true, GT>(p, s_p, ColorGeom{}, u, v, cl, s_tab, s_top, bitmap, cnt);
    }
    publish_counts(cnt, entered, counters);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(&counters[5], (unsigned long long)cl.lds_words * 4ull);
}

// ---------------------------------------------------------------------------------------
// Several renderings of the same model in one launch.  The tracking loop raycasts the model at every pyramid level
// that has ICP iterations (main.cpp:280-288: 640x480, 160x120, 80x60), and a coarse level takes as long as the
// full-resolution one: the march is a chain of ~150 dependent misses whatever the number of rays (DESIGN.md 5.2;
// measured 0.168 / 0.147 / 0.167 ms for levels 0 / 2 / 3).  One grid over the workgroups of all levels lets the
// chains overlap: 0.465 -> 0.274 ms (S_room), 0.452 -> 0.255 ms (S_full), scripts/raycast_levels.py.  Each pixel runs raycast_pixel unchanged, so every image is
// bit-identical to its own kfx_raycast_sdf call.
// ---------------------------------------------------------------------------------------
constexpr int RAY_MAX_LEVELS = 8;
struct RayLevel {
    unsigned char *dptr, *nptr, *iptr;
    size_t dpitch, npitch, ipitch;
    int w, h;
    Intr K;
    unsigned char* vptr;       // optional vertex map of the rendering: DepthToVbo(depth, K) (cu_depth_tools.cu:59-70), or null
    size_t vpitch;
    int first_block, blocks_x; // this level's workgroups are [first_block, next level's first_block), row-major
    int sparse;                // 0, or rays per wave (a strip of one pixel row, the other lanes idle); workgroup = 2 x 2 strips
};
struct RayLevels {
    RayLevel lv[RAY_MAX_LEVELS];
    int n;
};

// the level of workgroup `block` of the launch (uniform)
__device__ __forceinline__ const RayLevel& level_of(const RayLevels& L, const int block)
{
    int l = 0;
    for (int k = 1; k < L.n; ++k)
        if (block >= L.lv[k].first_block) l = k;
    return L.lv[l];
}
// the launch's parameters with a level's images and intrinsics
__device__ __forceinline__ RayParams level_params(const RayParams& base, const RayLevel& lv)
{
    RayParams p = base;
    p.dptr = lv.dptr; p.nptr = lv.nptr; p.iptr = lv.iptr;
    p.dpitch = lv.dpitch; p.npitch = lv.npitch; p.ipitch = lv.ipitch;
    p.w = lv.w; p.h = lv.h;
    p.K = lv.K;
    return p;
}
// the application's DepthToVbo(ray_v[l], ray_d[l], K[l]) (main.cpp:286) for a pixel whose depth image holds kz: depth_vertex
__device__ __forceinline__ void write_vertex(const RayLevel& lv, const RayParams& p, const int u, const int v, const float kz)
{
    if (lv.vptr && u < p.w && v < p.h) reinterpret_cast<float4*>(lv.vptr + (size_t)v * lv.vpitch)[u] = depth_vertex(p.K, kz, u, v);
}

template <typename CELL>
__global__ __launch_bounds__(256) void k_raycast_sdf_levels(const RayParams base, const RayLevels L)
{
    const RayLevel& lv = level_of(L, (int)blockIdx.x);
    const RayParams p = level_params(base, lv);
    const int b = (int)blockIdx.x - lv.first_block;
    int u, v;
    if (!ray_lane_pixel(p, lv.sparse, b % lv.blocks_x, b / lv.blocks_x, u, v)) return;
    write_vertex(lv, p, u, v, raycast_pixel<CELL, false>(p, ColorGeom{}, u, v));
}

template <typename CELL>
__global__ __launch_bounds__(256) void k_raycast_sdf_levels_classes(const RayParams base, const RayLevels L, const ClassView cl)
{
    extern __shared__ unsigned s_tab[];
    __shared__ RayParams s_p;
    __shared__ TopLevels s_top;
    __shared__ int s_any[4];   // (workgroup_any: one word per wave of the 256-thread workgroup)
    const RayLevel& lv = level_of(L, (int)blockIdx.x);
    const RayParams p = level_params(base, lv);
    if (threadIdx.x == 0) s_p = p;
    const int b = (int)blockIdx.x - lv.first_block;
    int u, v;
    const bool carries = ray_lane_pixel(p, lv.sparse, b % lv.blocks_x, b / lv.blocks_x, u, v);
    // as k_raycast_sdf_classes: a workgroup without a ray in the box leaves before the prologue (every thread reaches the barrier)
    const bool pixel = carries && u < p.w && v < p.h;
    float kz = __builtin_nanf("");   // what raycast_pixel_classes returns for a ray that hits nothing
    if (!workgroup_any(pixel && enters(ray_box(p, u, v)), s_any)) {
        if (!pixel) return;
        write_no_hit(ray_out(p, u, v));
    } else {
        classes_stage(cl, s_tab, s_top);   // before any lane leaves (barrier inside)
        if (!carries) return;
        kz = raycast_pixel_classes<CELL, false>(p, s_p, ColorGeom{}, u, v, cl, s_tab, s_top);
    }
    write_vertex(lv, p, u, v, kz);
}

// ---------------------------------------------------------------------------------------
// The colour image of any rendering (kfx_raycast_color_hits, include/kfx_color.h).  The colour variant of RaycastSdf differs
// from the grey one in one value per hit pixel, colorVol.GetUnitsTrilinearClamped(c_w + ray_w * depth) (write_ray), which
// depends on the pixel, the pose, the intrinsics and the depth the march stored -- so any march (plain, class tables, all
// levels in one launch) renders colour by being followed by this pass: one grid over the pixels of all levels, laid out as
// k_raycast_sdf_levels lays them out (dense 64 x 4 pixel workgroups).  The position is ray_box()'s and the sample
// trilinear<RayC32>'s, the expressions of write_ray in the same translation unit: in exact numerics the image is
// k_raycast_sdf<CELL, true>'s bit for bit.  Pixels without a hit keep the 0 the march wrote.
// ---------------------------------------------------------------------------------------
struct ColorHitLevel {
    const unsigned char* dptr;
    unsigned char* iptr;
    size_t dpitch, ipitch;
    int w, h;
    Intr K;
    int first_block, blocks_x; // this level's workgroups are [first_block, next level's first_block), row-major
};
struct ColorHitLevels {
    ColorHitLevel lv[RAY_MAX_LEVELS];
    int n;
};

__global__ __launch_bounds__(256) void k_raycast_color_hits(const Pose T, const ColorGeom cv, const ColorHitLevels L)
{
    int l = 0;
    for (int k = 1; k < L.n; ++k)
        if ((int)blockIdx.x >= L.lv[k].first_block) l = k;
    const ColorHitLevel& lv = L.lv[l];
    const int b = (int)blockIdx.x - lv.first_block;
    const int u = (b % lv.blocks_x) * 64 + (int)(threadIdx.x & 63), v = (b / lv.blocks_x) * 4 + (int)(threadIdx.x >> 6);
    if (u >= lv.w || v >= lv.h) return;
    const float depth = reinterpret_cast<const float*>(lv.dptr + (size_t)v * lv.dpitch)[u];
    if (depth > 0) { // (a miss holds NaN)
        RayParams p{};   // ray_box reads the pose and the intrinsics for c_w / ray_w; its slab test is not used here
        p.T = T;
        p.K = lv.K;
        const RayBox r = ray_box(p, u, v);
        reinterpret_cast<float*>(lv.iptr + (size_t)v * lv.ipitch)[u] = trilinear<RayC32>(cv, r.c_w + r.ray_w * depth);
    }
}

// ---------------------------------------------------------------------------------------
// Exact multi-GPU march ("exact variant").  The volume is split into Z-slabs; a ray's
// march state (lambda, last_sdf, delta) is carried from slab to slab in ray order, so every sample is
// taken at exactly the position, and from exactly the cells, of the single-volume march.  `p` describes
// the FULL volume's geometry with a virtual base pointer (local storage - z_offset planes), so
// trilinear() / gradient() address global plane indices unchanged.  A rank advances a ray while the
// trilinear base cell iz of the current sample lies in the cells it owns, [own_lo, own_hi), and the
// planes it needs are stored locally, [avail_lo, avail_hi).
// State: 9 dense planes of h*w floats (structure of arrays): 0 lambda, 1 last_sdf, 2 delta, 3 status,
// 4 touched-this-round, 5-7 normal, 8 shade.  status: 0 marching, 1 hit (final), 2 miss (final),
// 3 hit found, normal pending (computed by the rank that owns the gradient's base plane).  A hit's depth is
// its lambda.  Exactly one rank touches a pixel per round (ownership is disjoint), so the host merges the
// ranks' states with one integer SUM all-reduce of the touched pixels' planes 0-4.
// ---------------------------------------------------------------------------------------
struct SlabRay {
    // State of tile t (rows [t R, (t + 1) R) of the image, pixel q = (v - t R) w + u of it): march planes 0-3 at
    // state + (t * 4 + k) * P + q -- what travels with a ray: one contiguous message per tile --, normal / shade planes 5-8 at
    // result + (t * 4 + k - 5) * P + q.  touched (plane 4; null: not kept): the dense state's, for ONE tile.  One tile of R = h rows with
    // P = w h, touched = state + 4 P and result = state + 5 P is the dense [9][h w] layout of kfx_raycast_sdf_slab.
    // packed: THREE march planes per tile, at state + (t * 3 + k) * P + q: lambda, last_sdf and delta-or-status -- a marching ray's
    // delta (positive: the caller guarantees a positive truncation distance and voxel size), or -status of a ray that is not
    // marching (-1 hit, -2 miss, -3 hit awaiting its normal: such a ray's delta is never read again).  12 bytes per ray and hop
    // (SURVEY 8(e)); the received snapshots have the same layout.
    float* state;
    float* touched;
    float* result;
    int packed;
    // normals_here: a hit's normal is evaluated by whichever rank holds the hit (its finder, or a rank that adopted it) as soon as the
    // three planes of the gradient stencil are STORED there, ghost planes included -- they hold the owner's bits; else only by the
    // rank that OWNS the stencil's base plane (the hit travels there in the hand-over's last stage)
    int normals_here;
    size_t P;           // plane stride in pixels (>= R w)
    int R;              // rows per tile
    int v0, v1;         // rows this launch processes
    int* fin;           // optional, dense w h: set where THIS launch gives a ray its final status (and, with claim_misses, where
    int claim_misses;   //   the initialisation finds a ray that never enters the box: one rank answers for those)
    int own_lo, own_hi; // owned trilinear base cells (global plane indices)
    int avail_lo, avail_hi; // planes stored locally (global indices)
    int init;           // 1: (re)initialise the state from the ray / box intersection
    // Snapshots of the same rays received from the two neighbour ranks (march planes 0-3 as above; null: none): before marching, a
    // ray takes a neighbour's snapshot when that one is NEWER than its own and still under way (kfx_slab_raycast_exact_tiled).
    // adopt_tile_major: the buffers hold every tile ([tiles][4][P]) instead of just the tile of this launch ([4][P]).
    const float* adopt_lo;
    const float* adopt_hi;
    int adopt_tile_major;
};

// Snapshots of one march order by progress: status 1 / 2 (final) after 3 (hit, normal pending) after 0 (marching), and of two
// marching snapshots the one with the larger lambda is later (every step adds a positive delta).
__device__ __forceinline__ int snapshot_order(float status) { return status == 0.0f ? 0 : (status == 3.0f ? 1 : 2); }

// the z of a sample's base plane and of a gradient's: one axis of cell_of() (with the hardware division) and of gradient_base(),
// sampling.h -- stated here again: a per-axis helper under these and gradient_base() reorders the dense kernels' instructions
__device__ __forceinline__ int cell_z(const RayParams& p, const V3 pos_w)
{
    const float pfz = ((pos_w.z - p.vol.bmin.z) / p.size.z) * p.dims1.z;
    return (int)fmaxf(fminf(p.hi2.z, floorf(pfz)), 0.f);
}
__device__ __forceinline__ int grad_cell_z(const RayParams& p, const V3 pos_w)
{
    const float pfz = ((pos_w.z - p.vol.bmin.z) / p.size.z) * p.dims1.z;
    return (int)fmaxf(fminf(p.hi2.z, floorf(pfz)), 1.f);
}

// COLOR (include/kfx_slab_color.h): the rank that finalises a hit writes the colour volume's sample at the hit into the shade plane
// instead of the Phong shade -- write_ray<.., COLOR>'s expression on the slab's ColorGeom: the full colour volume's geometry over a
// virtual base pointer, as p is for the SDF volume.  The colour volume has the SDF volume's dimensions and box, so that geometry is
// p's own but for where the cells lie (SlabColor: the kernel carries no second copy of the box in scalar registers).  The colour
// travels where the shade travels.
struct SlabColor { unsigned char* ptr; size_t pitch, img_pitch; int off32; };
__device__ __forceinline__ ColorGeom slab_color_geom(const RayParams& p, const SlabColor& sc)
{
    ColorGeom cv;
    cv.vol = p.vol;
    cv.vol.ptr = sc.ptr; cv.vol.pitch = sc.pitch; cv.vol.img_pitch = sc.img_pitch;
    cv.size = p.size; cv.dims1 = p.dims1; cv.hi2 = p.hi2; cv.inv_size = p.inv_size;
    cv.fastdiv = p.fastdiv; cv.off32 = sc.off32;
    return cv;
}

template <typename CELL, bool COLOR>
__global__ __launch_bounds__(256) void k_raycast_sdf_slab(const RayParams p, const SlabRay sl, const SlabColor sc)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int u = blockIdx.x * 64 + (wv & 1) * 32 + (lane & 31); // wave = 32 x 2 pixels, as k_raycast_sdf's default
    const int v = sl.v0 + blockIdx.y * 4 + (wv >> 1) * 2 + (lane >> 5);
    if (u >= p.w || v >= sl.v1) return;
    const size_t plane = sl.P;
    const int tile = v / sl.R;
    const size_t q = (size_t)(v - tile * sl.R) * p.w + u;
    const int NP = sl.packed ? 3 : 4;
    float* st = sl.state + (size_t)tile * NP * plane + q;   // plane k at st[k * plane]
    float* rs = sl.result + (size_t)tile * 4 * plane + q;  // normal x / y / z, shade

    const RayBox box = ray_box(p, u, v);
    const V3 c_w = box.c_w, ray_c = box.ray_c, ray_w = box.ray_w;
    const float max_tmin = box.max_tmin, min_tmax = box.min_tmax;

    float lambda, last_sdf, delta, status;
    if (sl.init) {
        lambda = max_tmin;
        last_sdf = __builtin_nanf("");
        delta = 0.f;
        status = (max_tmin < min_tmax) ? 0.f : 2.f;
        rs[0] = 0.f; rs[plane] = 0.f; rs[2 * plane] = 0.f; rs[3 * plane] = 0.f;
        if (sl.fin) sl.fin[(size_t)v * p.w + u] = (sl.claim_misses && status == 2.f) ? 1 : 0;
    } else {
        lambda = st[0]; last_sdf = st[plane]; delta = st[2 * plane];
        if (sl.packed) { status = delta < 0.f ? -delta : 0.f; delta = delta < 0.f ? 0.f : delta; }
        else status = st[3 * plane];
    }
    // a neighbour's newer, still open snapshot of this ray replaces the rank's own (a stale copy is never advanced: its position
    // lies in planes of a rank the ray has left, and final snapshots stay with the rank that finalised them)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float* src = k ? sl.adopt_hi : sl.adopt_lo;
        if (!src) continue;
        src += (sl.adopt_tile_major ? (size_t)tile * NP * plane : (size_t)0) + q;
        const float n_code = src[2 * plane];
        const float n_status = sl.packed ? (n_code < 0.f ? -n_code : 0.f) : src[3 * plane];
        if (!(n_status == 0.f || n_status == 3.f)) continue;
        const float n_lambda = src[0];
        const int on = snapshot_order(n_status), om = snapshot_order(status);
        if (on > om || (on == 0 && om == 0 && n_lambda > lambda)) {
            lambda = n_lambda; last_sdf = src[plane]; delta = (sl.packed && n_code < 0.f) ? 0.f : n_code; status = n_status;
        }
    }
    const float lambda_in = lambda, status_in = status;

    if (status == 0.f) {
        const float min_delta = p.voxel.x;
        while (true) {
            if (!(lambda < min_tmax)) { status = 2.f; break; }
            const V3 pos = c_w + ray_w * lambda;
            const int iz = cell_z(p, pos);
            if (iz < sl.own_lo || iz >= sl.own_hi || iz < sl.avail_lo || iz + 1 >= sl.avail_hi) break; // another rank's sample
            const float sdf = trilinear<CELL>(p, pos);
            if (sdf <= 0) {
                if (last_sdf > 0) {
                    if (p.subpix) lambda = lambda + delta * sdf / (last_sdf - sdf);
                    status = 3.f;
                } else {
                    status = 2.f;
                }
                break;
            }
            delta = march_step(sdf, min_delta, p.trunc);
            lambda += delta;
            last_sdf = sdf;
        }
    }
    if (status == 3.f) { // hit: the rank owning the gradient's base plane gz evaluates the normal
        const V3 pos = c_w + ray_w * lambda;
        const int gz = grad_cell_z(p, pos);
        if ((sl.normals_here || (gz >= sl.own_lo && gz < sl.own_hi)) && gz - 1 >= sl.avail_lo && gz + 1 < sl.avail_hi) {
            const V3 n_c = normal_c<CELL>(p, pos);
            rs[0] = n_c.x; rs[plane] = n_c.y; rs[2 * plane] = n_c.z;
            // The finaliser always holds the colour sample's planes: the sample's base plane is iz = clamp(floor(pfz), 0, d - 2), the
            // gradient's gz = clamp(floor(pfz), 1, d - 2) with the same pfz -- the colour volume has the SDF volume's dimensions and box
            // (check_color_slab) -- so iz is gz or gz - 1 and planes iz, iz + 1 lie inside [gz - 1, gz + 1], which the test above has
            // just found stored; with and without normals_here.
            if constexpr (COLOR) rs[3 * plane] = trilinear<RayC32>(slab_color_geom(p, sc), pos);
            else rs[3 * plane] = phong(ray_c * lambda, n_c);
            status = 1.f;
        }
    }
    const bool changed = lambda != lambda_in || status != status_in;
    st[0] = lambda; st[plane] = last_sdf;
    if (sl.packed) st[2 * plane] = status == 0.f ? delta : -status;
    else { st[2 * plane] = delta; st[3 * plane] = status; }
    if (sl.touched) sl.touched[q] = changed ? 1.0f : 0.0f;
    if (sl.fin && changed && (status == 1.f || status == 2.f)) sl.fin[(size_t)v * p.w + u] = 1;
}

// state -> the three output images (hit: depth / normal / shade; otherwise NaN / 0 / 0)
__global__ __launch_bounds__(256) void k_raycast_state_to_images(const RayParams p, const float* __restrict__ state)
{
    int u, v;
    pixel_xy(u, v);
    if (u >= p.w || v >= p.h) return;
    const size_t plane = (size_t)p.w * p.h;
    const float* st = state + (size_t)v * p.w + u;
    const float depth = st[0];
    const bool hit = st[3 * plane] == 1.f && depth > 0.f;
    const RayOut o = ray_out(p, u, v);
    if (hit) write_hit(o, depth, make_float4(st[5 * plane], st[6 * plane], st[7 * plane], 1.0f), st[8 * plane]);
    else write_no_hit(o);
}

} // namespace kfx

using namespace kfx;

// argument checks of one output image set + volume, and the kernel parameters they give
template <typename CELL>
static int ray_params(RayParams& p, const kfx_image* depth, const kfx_image* norm, const kfx_image* img,
                      const kfx_volume* vol, const float T_wc[12], const float K[4], float near,
                      float far, float trunc_dist, int subpix)
{
    if (!T_wc || !K) return set_error(KFX_E_NULL, "RaycastSdf: null argument");
    if (int e = check_render_images(depth, norm, img, img, "RaycastSdf")) return e;
    // the gradient stencil reads cells [1-1, (dim-2)+1] (Volume.h:271-273)
    if (int e = check_volume(vol, CELL::BYTES, 3, VOLUME_MAX_DIM, "RaycastSdf")) return e;
    set_geometry(p, vol);
    set_voxel_size(p, vol);
    ray_fill(p, depth, norm, img, T_wc, K, near, far, trunc_dist, subpix);
    return 0;
}

// The class-table march's view of a summary for a launch on `vol` with camera T_wc: brings the tables up to date on `stream`,
// evaluates the margin that covers the affine cell estimate, reports the LDS bytes.  *usable = 0: march plainly (the margin
// would be too wide, or trunc is not positive).
// Half cells (SDF_h): class 1 means "every cell holds vref = trunc rounded to half" -- what the plain march samples in untouched
// free space -- and the fast-numerics band is KFX_SUMMARY_HALF_BAND (include/kfx.h) instead of 1e-5.
// Tables larger than the LDS budget (fp32 or half cells at ~2000^3), or KFX_RAYCAST_GLOBAL_TABLES=1: the global-table mode
// (ClassView::global): a 16^3-cell fine level, the 32^3-cell level and the two derived levels in global memory, the latter two
// staged.  The levels march (RaycastSdfLevels) runs the plain march in that mode (*usable = 2: the caller decides).
// allow_global = false (the levels call, which has no global-table kernel): where the global-table mode would be needed, return
// unusable before any table is built and before the plain / table choice is touched.
template <typename CELL>
static int class_view(ClassView& cl, size_t* lds_bytes, int* usable, kfx_sdf_summary* summary, const kfx_volume* vol, const RayParams& p, kfx_stream stream,
                      bool allow_global = true)
{
    *usable = 0;
    if (int e = summary_view_offset(summary, vol, &cl.ox, &cl.oy, &cl.oz)) return e;
    if (!(p.trunc > 0.f) || !(p.trunc < __builtin_inff())) return 0;
    static const int kb_env = env_int("KFX_RAYCAST_CLASS_KB", 16, 1, 60);
    static const int gt_env = env_int("KFX_RAYCAST_GLOBAL_TABLES", 0);
    static const int top_env = env_int("KFX_RAYCAST_TOP_LEVELS", 2, 0, 2);
    int fine = 3;
    for (; fine < 5; ++fine) {
        summary_class_layout(summary, fine, cl);
        if ((size_t)cl.words * 4 <= (size_t)kb_env * 1024) break;
    }
    // the coarser levels (64^3 cells where the 32^3-cell level has more than one entry along some axis, 128^3 cells likewise on
    // top of that): built in global memory behind the 32^3-cell level (by the table build's last workgroup, or -- global-table
    // mode -- by launches of their own) and staged with the rest
    auto top_levels = [&](int& w6, int& w7) {
        summary_class_layout(summary, fine, cl);
        cl.nx5 = ceil_div(summary->w, 32); cl.nz5 = ceil_div(summary->d, 32);
        ClassLevel l6, l7;
        summary_top_layout(cl, l6, l7, w6, w7);
        const int nx6 = (cl.nx5 + 1) >> 1, nz6 = (cl.nz5 + 1) >> 1;
        cl.top_n = 0;
        if (cl.nx5 > 1 || cl.coarse.ny > 1 || cl.nz5 > 1) cl.top_n = 1;
        if (cl.top_n && (nx6 > 1 || l6.ny > 1 || nz6 > 1)) cl.top_n = 2;
        if (cl.top_n > top_env) cl.top_n = top_env;
    };
    int w6, w7;
    top_levels(w6, w7);
    // the launch asks for the staged tables PLUS the derived levels PLUS the kernels' static LDS (RayParams, TopLevels, the
    // levels kernel's table): the whole must stay below the 64 KiB a launch may have (round-4 advice)
    const size_t lds_static = sizeof(RayParams) + sizeof(TopLevels) + 2048;
    const int derived = (cl.top_n > 0 ? w6 : 0) + (cl.top_n > 1 ? w7 : 0);
    cl.global = gt_env > 0 || (size_t)cl.words * 4 > 60 * 1024 || (size_t)(cl.words + derived) * 4 + lds_static > 64 * 1024;
    if (cl.global) {
        fine = 4;
        top_levels(w6, w7);
        cl.top_first = cl.words;
        cl.lds_words = (cl.top_n > 0 ? w6 : 0) + (cl.top_n > 1 ? w7 : 0);
        if ((size_t)cl.lds_words * 4 + lds_static > 64 * 1024) return 0;
    } else {
        cl.top_first = 0;
        cl.lds_words = cl.words + derived;
    }
    if (cl.global && !allow_global) return 0;
    const bool half = CELL::BYTES == 4;
    const float vref = half ? __half2float(__float2half_rn(p.trunc)) : p.trunc;
    const float tol = math_mode() == KFX_MATH_FAST ? (half ? KFX_SUMMARY_HALF_BAND : 1e-5f) : 0.f;
    // Worth it?  The march through the tables costs ~8 % per sampled step (table look-ups, staging); it pays where a fair part
    // of the volume can be crossed without sampling: at least a quarter of the 32^3-cell entries of class != 0.  Every table
    // build publishes that count in a host-visible ring; the choice is made from the count of the build BEFORE THE PREVIOUS ONE
    // (two frames old: finished long ago, so its slot carries its stamp at the first look below) -- it only steers a choice between two
    // kernels that render the same images, but in fast numerics "the same" means within tolerance, so the choice is made a
    // function of the sequence of calls, not of how far the GPU happens to have got (round-3 advice).  Exact numerics on a
    // running stream, where only never-observed space qualifies, fall back to the plain march this way; while the choice is
    // "plain" the tables are rebuilt on every 8th call only.  KFX_RAYCAST_SUMMARY=1 always uses the tables, -1 never.
    static const int force_env = env_int("KFX_RAYCAST_SUMMARY", 0);
    if (force_env < 0) return 0;
    const bool steer = force_env == 0 && summary->h_skippable;
    if (steer && summary->plain_calls && (summary->plain_calls++ % 8u) != 0u) return 0;   // still plain: no build, no look
    if (int e = summary_classes_prepare(summary, tol, vref, fine, (hipStream_t)stream, cl.global)) return e;
    if (steer && summary->builds >= 3) {
        // builds - 1 is the one just issued (or the last one).  Build builds - 3 has published long ago as a rule: its slot
        // carries its stamp at the first look.  With the host far ahead of the stream the looks go on, the thread yielding in
        // between -- 2^20 of them at most (a second or so), then the stream is synchronised and the slot looked at once more; a
        // slot that does not carry the stamp even then (a build on a stream that does not make progress) is an error, never a count.
        const unsigned ref = summary->builds - 3;
        const unsigned long long* slot = summary->h_skippable + summary_ring_index(ref);
        int known = 0;
        const int seen = summary_ring_wait(
            ref, 1ull << 20,
            [&]() {
                const uint64_t v = __atomic_load_n(slot, __ATOMIC_ACQUIRE);
                if (summary_ring_slot_stamp(v) != summary_ring_stamp(ref)) std::this_thread::yield();
                return v;
            },
            [&]() { (void)hipStreamSynchronize((hipStream_t)stream); }, &known);
        if (seen < 0) return set_error(KFX_E_TIMEOUT, "RaycastSdf(tracked): the class-table build the choice of the march rests on has not published its count");
        if ((long long)known * 4 < summary->n_coarse) {   // less than a quarter
            if (!summary->plain_calls) summary->plain_calls = 1;
            return 0;
        }
        summary->plain_calls = 0;
    }
    cl.C = summary->C;
    cl.vref = vref;
    // class 3 needs equal steps for a vref and a NaN sample: max(vref, min_delta) = trunc (fp32: trunc >= min_delta; half cells
    // only where trunc is a half value)
    cl.amb_ok = fmaxf(vref, p.voxel.x) == p.trunc ? 1 : 0;
    cl.tol = tol;
    // margin: |cell_of()'s coordinate - the affine estimate| per axis, from the roundings of both (u = 2^-24):
    //   cell_of:   pos = c + ray lambda (2 roundings of magnitudes <= |pos| + |c|), - bmin, / size, * dims1
    //   estimate:  A = (c - bmin) sc (3 roundings), B = ray sc (2), fma(B, lambda, A) (1); and the run's far side
    //              (bound - A) / B, whose error in this axis' coordinate is 3 u (|bound| + |A|) whatever B is
    const double u24 = 1.0 / 16777216.0;
    double eps = 0.0;
    const float bmin[3] = {p.vol.bmin.x, p.vol.bmin.y, p.vol.bmin.z}, bmax[3] = {p.vol.bmax.x, p.vol.bmax.y, p.vol.bmax.z};
    const float size[3] = {p.size.x, p.size.y, p.size.z}, dims1[3] = {p.dims1.x, p.dims1.y, p.dims1.z};
    const float cw[3] = {p.T.m[3], p.T.m[7], p.T.m[11]};
    for (int a = 0; a < 3; ++a) {
        if (!(size[a] > 0.f)) return 0;
        const double sc = (double)dims1[a] / size[a];
        const double pmax = std::fmax(std::fabs((double)bmin[a]), std::fabs((double)bmax[a])), ca = std::fabs((double)cw[a]);
        const double A = std::fabs(((double)cw[a] - bmin[a]) * sc);
        const double t = sc * (3.0 * pmax + 2.0 * ca + size[a]) * u24 + 2.0 * dims1[a] * u24;
        const double e = u24 * (3.0 * A + 2.0 * sc * (pmax + ca) + dims1[a]) + 3.0 * u24 * (dims1[a] + A);
        eps = std::fmax(eps, t + e);
    }
    eps *= 2.0;   // twice the bound
    if (!(eps < 0.05)) return 0;
    cl.eps = (float)std::fmax(eps, 1e-4);
    *lds_bytes = (size_t)cl.lds_words * sizeof(unsigned);
    *usable = 1;
    return 0;
}

// The march a class_view() result selects, launched on `grid`: through the tables (`global`: the global-table kernel, `lds`: the
// one with all levels in LDS; a... are their arguments after (p, cl)), or, where the tables are not usable, plain().
template <typename PLAIN, typename... A>
static int launch_march(const char* what, int usable, const ClassView& cl, size_t cl_bytes, dim3 grid, kfx_stream stream, const RayParams& p,
                        void (*global)(RayParams, ClassView, A...), void (*lds)(RayParams, ClassView, A...), PLAIN plain, A... a)
{
    if (usable) hipLaunchKernelGGL(cl.global ? global : lds, grid, dim3(256), cl_bytes, (hipStream_t)stream, p, cl, a...);
    else plain();
    return check_launch(what);
}

template <typename CELL>
static int raycast_levels_launch(int n_levels, const kfx_image* const* depth, const kfx_image* const* norm, const kfx_image* const* img,
                                 const kfx_image* const* vbo, const kfx_volume* vol, const float T_wc[12], const float* K, float near, float far,
                                 float trunc_dist, int subpix, kfx_stream stream, kfx_sdf_summary* summary = nullptr)
{
    if (n_levels < 0 || n_levels > RAY_MAX_LEVELS) return set_error(KFX_E_RANGE, "RaycastSdf(levels): number of levels");
    if (!depth || !norm || !img || !K) return set_error(KFX_E_NULL, "RaycastSdf(levels): null argument");
    RayParams base{};
    RayLevels L{};
    int blocks = 0;
    for (int l = 0; l < n_levels; ++l) { // (coarse levels first was tried: no faster)
        RayParams p;
        if (int e = ray_params<CELL>(p, depth[l], norm[l], img[l], vol, T_wc, K + 4 * l, near, far, trunc_dist, subpix)) return e;
        if (p.w == 0 || p.h == 0) continue; // an empty level launches nothing, as kfx_raycast_sdf
        RayLevel& lv = L.lv[L.n++];
        lv.dptr = p.dptr; lv.nptr = p.nptr; lv.iptr = p.iptr;
        lv.dpitch = p.dpitch; lv.npitch = p.npitch; lv.ipitch = p.ipitch;
        lv.w = p.w; lv.h = p.h;
        lv.K = p.K;
        lv.vptr = nullptr;
        lv.vpitch = 0;
        if (vbo && vbo[l]) {
            const kfx_image* vb = vbo[l];
            if (int e = check_image(vb, 16, (size_t)p.w, (size_t)p.h, "RaycastSdf(levels): vertex map")) return e;
            lv.vptr = (unsigned char*)vb->ptr;
            lv.vpitch = vb->pitch;
        }
        lv.first_block = blocks;
        static const int sparse_env = [] { const int v = env_int("KFX_RAYCAST_SPARSE", 16); return (v == 8 || v == 16 || v == 32) ? v : 0; }();
        lv.sparse = (long long)p.w * p.h <= 160 * 120 ? sparse_env : 0; // coarse levels only: at full resolution dense waves are faster
        lv.blocks_x = lv.sparse ? ceil_div(p.w, 2 * lv.sparse) : ceil_div(p.w, 64);
        blocks += lv.blocks_x * (lv.sparse ? ceil_div(p.h, 2) : ceil_div(p.h, 4));
        base = p;
    }
    if (summary && summary->cell_bytes != CELL::BYTES)
        return set_error(KFX_E_SHAPE, "RaycastSdf(levels, tracked): the summary was created for the other cell type (kfx_sdf_summary_create / _create_h)");
    if (L.n == 0) return 0;
    if (summary) {
        ClassView cl;
        size_t cl_bytes = 0;
        int usable = 0;
        if (int e = class_view<CELL>(cl, &cl_bytes, &usable, summary, vol, base, stream, false)) return e;
        if (usable) {   // (the global-table mode has no levels kernel: class_view said unusable, the plain march below)
            hipLaunchKernelGGL((k_raycast_sdf_levels_classes<CELL>), dim3(blocks), dim3(256), cl_bytes, (hipStream_t)stream, base, L, cl);
            return check_launch("kfx_raycast_sdf_levels_tracked");
        }
    }
    hipLaunchKernelGGL((k_raycast_sdf_levels<CELL>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, base, L);
    return check_launch("kfx_raycast_sdf_levels");
}

template <typename CELL>
static int raycast_launch(const kfx_image* depth, const kfx_image* norm, const kfx_image* img,
                          const kfx_volume* vol, const float T_wc[12], const float K[4], float near,
                          float far, float trunc_dist, int subpix, kfx_stream stream, const kfx_volume* colorvol = nullptr,
                          kfx_sdf_summary* summary = nullptr)
{
    RayParams p;
    if (int e = ray_params<CELL>(p, depth, norm, img, vol, T_wc, K, near, far, trunc_dist, subpix)) return e;
    if (summary && summary->cell_bytes != CELL::BYTES)
        return set_error(KFX_E_SHAPE, "RaycastSdf(tracked): the summary was created for the other cell type (kfx_sdf_summary_create / _create_h)");
    if (p.w == 0 || p.h == 0) return 0;

    const dim3 grid = ray_tiling(p);
    ColorGeom cv{};
    if (colorvol) {
        if (int e = check_volume(colorvol, 4, 2, VOLUME_ANY_DIM, "RaycastSdf(colour)")) return e;
        set_geometry(cv, colorvol);
        hipLaunchKernelGGL((k_raycast_sdf<CELL, true>), grid, dim3(256), 0, (hipStream_t)stream, p, cv);
    } else if (summary) {
        ClassView cl;
        size_t cl_bytes = 0;
        int usable = 0;
        if (int e = class_view<CELL>(cl, &cl_bytes, &usable, summary, vol, p, stream)) return e;
        return launch_march("kfx_raycast_sdf_tracked", usable, cl, cl_bytes, grid, stream, p, k_raycast_sdf_classes<CELL, true>, k_raycast_sdf_classes<CELL, false>,
                            [&] { hipLaunchKernelGGL((k_raycast_sdf<CELL, false>), grid, dim3(256), 0, (hipStream_t)stream, p, cv); });
    } else {
        hipLaunchKernelGGL((k_raycast_sdf<CELL, false>), grid, dim3(256), 0, (hipStream_t)stream, p, cv);
    }
    return check_launch("kfx_raycast_sdf");
}

extern "C" int kfx_raycast_sdf(const kfx_image* depth, const kfx_image* norm, const kfx_image* img,
                               const kfx_volume* vol, const float T_wc[12], const float K[4], float near,
                               float far, float trunc_dist, int subpix, kfx_stream stream)
{
    return raycast_launch<RayF32>(depth, norm, img, vol, T_wc, K, near, far, trunc_dist, subpix, stream);
}

// Parameters and grid of a count launch.  The image arguments of ray_params() only give the launch its size: nothing is written to them.
template <typename CELL>
static int count_params(RayParams& p, dim3& grid, const kfx_volume* vol, unsigned w, unsigned h, const float T_wc[12], const float K[4], float near, float far,
                        float trunc_dist, int subpix)
{
    kfx_image dummy = {(size_t)w * 16, (void*)(uintptr_t)16, w, h};
    if (int e = ray_params<CELL>(p, &dummy, &dummy, &dummy, vol, T_wc, K, near, far, trunc_dist, subpix)) return e;
    p.dptr = p.nptr = p.iptr = nullptr;
    grid = pixel_grid(p.w, p.h);
    return 0;
}

template <typename CELL>
static int raycast_count_launch(const kfx_volume* vol, unsigned w, unsigned h, const float T_wc[12], const float K[4], float near, float far,
                                float trunc_dist, int subpix, unsigned* d_bitmap, unsigned long long* d_counters, kfx_stream stream)
{
    if (!d_bitmap || !d_counters) return set_error(KFX_E_NULL, "kfx_raycast_sdf_count: null argument");
    RayParams p;
    dim3 grid;
    if (int e = count_params<CELL>(p, grid, vol, w, h, T_wc, K, near, far, trunc_dist, subpix)) return e;
    if (p.w == 0 || p.h == 0) return 0;
    hipLaunchKernelGGL(k_raycast_sdf_count<CELL>, grid, dim3(256), 0, (hipStream_t)stream, p, d_bitmap, d_counters);
    return check_launch("kfx_raycast_sdf_count");
}

extern "C" int kfx_raycast_sdf_count(const kfx_volume* vol, unsigned w, unsigned h, const float T_wc[12], const float K[4], float near, float far,
                                     float trunc_dist, int subpix, unsigned* d_bitmap, unsigned long long* d_counters, kfx_stream stream)
{
    return raycast_count_launch<RayF32>(vol, w, h, T_wc, K, near, far, trunc_dist, subpix, d_bitmap, d_counters, stream);
}

extern "C" int kfx_raycast_sdf_count_h(const kfx_volume* vol, unsigned w, unsigned h, const float T_wc[12], const float K[4], float near, float far,
                                       float trunc_dist, int subpix, unsigned* d_bitmap, unsigned long long* d_counters, kfx_stream stream)
{
    return raycast_count_launch<RayF16>(vol, w, h, T_wc, K, near, far, trunc_dist, subpix, d_bitmap, d_counters, stream);
}

template <typename CELL>
static int raycast_count_tracked_launch(const kfx_volume* vol, kfx_sdf_summary* summary, unsigned w, unsigned h, const float T_wc[12], const float K[4],
                                        float near, float far, float trunc_dist, int subpix, unsigned* d_bitmap, unsigned long long* d_counters,
                                        kfx_stream stream)
{
    if (!d_bitmap || !d_counters || !summary) return set_error(KFX_E_NULL, "kfx_raycast_sdf_count_tracked: null argument");
    RayParams p;
    dim3 grid;
    if (int e = count_params<CELL>(p, grid, vol, w, h, T_wc, K, near, far, trunc_dist, subpix)) return e;
    if (summary->cell_bytes != CELL::BYTES)
        return set_error(KFX_E_SHAPE, "kfx_raycast_sdf_count_tracked: the summary was created for the other cell type (kfx_sdf_summary_create / _create_h)");
    if (p.w == 0 || p.h == 0) return 0;
    ClassView cl;
    size_t cl_bytes = 0;
    int usable = 0;
    // a diagnostics call must not steer the calls that follow: class_view() advances the plain / table choice's call counter
    // (the tables it may build are a pure function of the summary: harmless)
    const unsigned plain_calls = summary->plain_calls;
    const int ce = class_view<CELL>(cl, &cl_bytes, &usable, summary, vol, p, stream);
    summary->plain_calls = plain_calls;
    if (ce) return ce;
    return launch_march("kfx_raycast_sdf_count_tracked", usable, cl, cl_bytes, grid, stream, p, k_raycast_sdf_classes_count<CELL, true>,
                        k_raycast_sdf_classes_count<CELL, false>,   // (plain: what the tracked call would launch)
                        [&] { hipLaunchKernelGGL(k_raycast_sdf_count<CELL>, grid, dim3(256), 0, (hipStream_t)stream, p, d_bitmap, d_counters); }, d_bitmap, d_counters);
}

extern "C" int kfx_raycast_sdf_count_tracked(const kfx_volume* vol, kfx_sdf_summary* summary, unsigned w, unsigned h, const float T_wc[12], const float K[4],
                                             float near, float far, float trunc_dist, int subpix, unsigned* d_bitmap, unsigned long long* d_counters,
                                             kfx_stream stream)
{
    return raycast_count_tracked_launch<RayF32>(vol, summary, w, h, T_wc, K, near, far, trunc_dist, subpix, d_bitmap, d_counters, stream);
}

extern "C" int kfx_raycast_sdf_count_tracked_h(const kfx_volume* vol, kfx_sdf_summary* summary, unsigned w, unsigned h, const float T_wc[12], const float K[4],
                                               float near, float far, float trunc_dist, int subpix, unsigned* d_bitmap, unsigned long long* d_counters,
                                               kfx_stream stream)
{
    return raycast_count_tracked_launch<RayF16>(vol, summary, w, h, T_wc, K, near, far, trunc_dist, subpix, d_bitmap, d_counters, stream);
}

extern "C" int kfx_raycast_sdf_tracked(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const kfx_volume* vol,
                                       kfx_sdf_summary* summary, const float T_wc[12], const float K[4], float near, float far,
                                       float trunc_dist, int subpix, kfx_stream stream)
{
    if (!summary) return set_error(KFX_E_NULL, "kfx_raycast_sdf_tracked: null summary");
    return raycast_launch<RayF32>(depth, norm, img, vol, T_wc, K, near, far, trunc_dist, subpix, stream, nullptr, summary);
}

extern "C" int kfx_raycast_sdf_tracked_h(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const kfx_volume* vol,
                                         kfx_sdf_summary* summary, const float T_wc[12], const float K[4], float near, float far,
                                         float trunc_dist, int subpix, kfx_stream stream)
{
    if (!summary) return set_error(KFX_E_NULL, "kfx_raycast_sdf_tracked_h: null summary");
    return raycast_launch<RayF16>(depth, norm, img, vol, T_wc, K, near, far, trunc_dist, subpix, stream, nullptr, summary);
}

extern "C" int kfx_raycast_sdf_h(const kfx_image* depth, const kfx_image* norm, const kfx_image* img,
                                 const kfx_volume* vol, const float T_wc[12], const float K[4], float near,
                                 float far, float trunc_dist, int subpix, kfx_stream stream)
{
    return raycast_launch<RayF16>(depth, norm, img, vol, T_wc, K, near, far, trunc_dist, subpix, stream);
}

// RaycastSdf(depth, norm, img, vol, colorVol, T_wc, K, near, far, trunc_dist, subpix) (cu_raycast.cu:119-196)
extern "C" int kfx_raycast_sdf_levels(int n_levels, const kfx_image* const* depth, const kfx_image* const* norm, const kfx_image* const* img,
                                      const kfx_image* const* vbo, const kfx_volume* vol, const float T_wc[12], const float* K, float near, float far,
                                      float trunc_dist, int subpix, kfx_stream stream)
{
    return raycast_levels_launch<RayF32>(n_levels, depth, norm, img, vbo, vol, T_wc, K, near, far, trunc_dist, subpix, stream);
}

extern "C" int kfx_raycast_sdf_levels_tracked(int n_levels, const kfx_image* const* depth, const kfx_image* const* norm, const kfx_image* const* img,
                                              const kfx_image* const* vbo, const kfx_volume* vol, kfx_sdf_summary* summary, const float T_wc[12],
                                              const float* K, float near, float far, float trunc_dist, int subpix, kfx_stream stream)
{
    if (!summary) return set_error(KFX_E_NULL, "kfx_raycast_sdf_levels_tracked: null summary");
    return raycast_levels_launch<RayF32>(n_levels, depth, norm, img, vbo, vol, T_wc, K, near, far, trunc_dist, subpix, stream, summary);
}

extern "C" int kfx_raycast_sdf_levels_h(int n_levels, const kfx_image* const* depth, const kfx_image* const* norm, const kfx_image* const* img,
                                      const kfx_image* const* vbo, const kfx_volume* vol, const float T_wc[12], const float* K, float near, float far,
                                      float trunc_dist, int subpix, kfx_stream stream)
{
    return raycast_levels_launch<RayF16>(n_levels, depth, norm, img, vbo, vol, T_wc, K, near, far, trunc_dist, subpix, stream);
}

extern "C" int kfx_raycast_sdf_levels_tracked_h(int n_levels, const kfx_image* const* depth, const kfx_image* const* norm, const kfx_image* const* img,
                                                const kfx_image* const* vbo, const kfx_volume* vol, kfx_sdf_summary* summary, const float T_wc[12],
                                                const float* K, float near, float far, float trunc_dist, int subpix, kfx_stream stream)
{
    if (!summary) return set_error(KFX_E_NULL, "kfx_raycast_sdf_levels_tracked_h: null summary");
    return raycast_levels_launch<RayF16>(n_levels, depth, norm, img, vbo, vol, T_wc, K, near, far, trunc_dist, subpix, stream, summary);
}

extern "C" int kfx_raycast_sdf_color(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const kfx_volume* vol,
                                     const kfx_volume* colorvol, const float T_wc[12], const float K[4], float near, float far,
                                     float trunc_dist, int subpix, kfx_stream stream)
{
    if (!colorvol) return set_error(KFX_E_NULL, "RaycastSdf(colour): null colour volume");
    return raycast_launch<RayF32>(depth, norm, img, vol, T_wc, K, near, far, trunc_dist, subpix, stream, colorvol);
}

// The colour image of renderings already marched (include/kfx_color.h): img[l](u, v) = colorvol's trilinear sample at the hit
// of pixel (u, v) of depth[l], for every pixel with depth > 0; one launch for all levels.
extern "C" int kfx_raycast_color_hits(int n_levels, const kfx_image* const* depth, const kfx_image* const* img, const kfx_volume* colorvol,
                                      const float T_wc[12], const float* K, kfx_stream stream)
{
    if (n_levels < 1 || n_levels > RAY_MAX_LEVELS) return set_error(KFX_E_RANGE, "RaycastSdf(colour pass): number of levels");
    if (!depth || !img || !colorvol || !T_wc || !K) return set_error(KFX_E_NULL, "RaycastSdf(colour pass): null argument");
    if (int e = check_volume(colorvol, 4, 2, VOLUME_ANY_DIM, "RaycastSdf(colour pass)")) return e;
    ColorHitLevels L{};
    int blocks = 0;
    for (int l = 0; l < n_levels; ++l) {
        const kfx_image *d = depth[l], *i = img[l];
        if (!d || !i || !d->ptr || !i->ptr) return set_error(KFX_E_NULL, "RaycastSdf(colour pass): null image");
        if (d->w != i->w || d->h != i->h) return set_error(KFX_E_SHAPE, "RaycastSdf(colour pass): depth and colour image of different sizes");
        if (d->w > 0x7fffffffu || d->h > 0x7fffffffu) return set_error(KFX_E_RANGE, "RaycastSdf(colour pass): image dimensions");
        if (int e = check_image(d, 4, 0, 0, "RaycastSdf(colour pass): depth image")) return e;
        if (int e = check_image(i, 4, 0, 0, "RaycastSdf(colour pass): colour image")) return e;
        if (d->w == 0 || d->h == 0) continue; // an empty level launches nothing
        ColorHitLevel& lv = L.lv[L.n++];
        lv.dptr = (const unsigned char*)d->ptr; lv.iptr = (unsigned char*)i->ptr;
        lv.dpitch = d->pitch; lv.ipitch = i->pitch;
        lv.w = (int)d->w; lv.h = (int)d->h;
        lv.K = Intr{K[4 * l], K[4 * l + 1], K[4 * l + 2], K[4 * l + 3]};
        lv.first_block = blocks;
        lv.blocks_x = ceil_div(lv.w, 64);
        const long long nb = (long long)lv.blocks_x * ceil_div(lv.h, 4);
        if (blocks + nb > 0x7fffffffLL) return set_error(KFX_E_RANGE, "RaycastSdf(colour pass): too many pixels");
        blocks += (int)nb;
    }
    if (L.n == 0) return 0;
    ColorGeom cv{};
    set_geometry(cv, colorvol);
    Pose T;
    for (int k = 0; k < 12; ++k) T.m[k] = T_wc[k];
    hipLaunchKernelGGL(k_raycast_color_hits, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T, cv, L);
    return check_launch("kfx_raycast_color_hits");
}

// Exact multi-GPU march: one round of a rank (see k_raycast_sdf_slab).  `vol` holds planes
// [slab->z_offset, slab->z_offset + vol->d) of the full volume described by `slab`; the rank owns the
// trilinear base cells [own_lo, own_hi).  `state` is KFX_RAY_STATE_PLANES dense planes of h*w floats; init != 0 starts the rays.
// colorvol (fp32 cells only): the rank's colour slab, the planes of `vol` of a colour volume with the SDF volume's geometry; the
// shade plane receives the colour of the hits this rank finalises.
template <typename CELL>
static int raycast_slab_launch(const SlabRay& geom, const kfx_volume* vol, const kfx_slab* slab, int own_lo, int own_hi,
                                    int w, int h, const float T_wc[12], const float K[4], float near, float far,
                                    float trunc_dist, int subpix, kfx_stream stream, const kfx_volume* colorvol = nullptr)
{
    if (!geom.state || !geom.result || !vol || !vol->ptr || !slab || !T_wc || !K) return set_error(KFX_E_NULL, "RaycastSdf(slab): null argument");
    if (colorvol) {
        if (int e = check_volume(colorvol, 4, 1, VOLUME_MAX_DIM, "RaycastSdf(slab, colour)")) return e;
        if (int e = check_color_slab(vol, colorvol, "RaycastSdf(slab, colour)")) return e;
    }
    if (w <= 0 || h <= 0 || geom.v1 <= geom.v0) return 0;
    if (geom.R < 1 || geom.v0 < 0 || geom.v1 > h || geom.P < (size_t)geom.R * (size_t)w) return set_error(KFX_E_SHAPE, "RaycastSdf(slab): tile geometry");
    if (slab->full_d < 3 || slab->z_offset + vol->d > slab->full_d || vol->w < 3 || vol->h < 3)
        return set_error(KFX_E_SHAPE, "RaycastSdf(slab): slab outside the full volume");
    if ((((uintptr_t)vol->ptr | vol->pitch | vol->img_pitch) & (CELL::BYTES - 1)) || (((uintptr_t)geom.state | (uintptr_t)geom.result | (uintptr_t)geom.fin) & 3))
        return set_error(KFX_E_ALIGN, "RaycastSdf(slab): alignment");
    RayParams p;
    // full-volume geometry, virtual base pointer (never dereferenced outside [avail_lo, avail_hi))
    const kfx_volume full = slab_full_volume(vol, slab);
    set_geometry(p, &full);
    set_voxel_size(p, &full);
    for (int i = 0; i < 12; ++i) p.T.m[i] = T_wc[i];
    p.K = Intr{K[0], K[1], K[2], K[3]};
    p.dptr = p.nptr = p.iptr = nullptr;
    p.dpitch = p.npitch = p.ipitch = 0;
    p.w = w;
    p.h = h;
    p.near = near;
    p.far = far;
    p.trunc = trunc_dist;
    p.subpix = subpix ? 1 : 0;
    p.tile_log2w = 3;
    p.wg_log2x = 1;
    SlabRay sl = geom;
    sl.own_lo = own_lo; sl.own_hi = own_hi;
    sl.avail_lo = (int)slab->z_offset; sl.avail_hi = (int)(slab->z_offset + vol->d);
    const dim3 grid = pixel_grid(w, sl.v1 - sl.v0);
    SlabColor sc{};
    if constexpr (CELL::BYTES == 8) {
        if (colorvol) {
            // the slab's ColorGeom: set_geometry on the full colour volume gives p's box members (equal dimensions and box:
            // check_color_slab) and the colour cells' own addressing
            const kfx_volume cfull = slab_full_volume(colorvol, slab);
            ColorGeom cv{};
            set_geometry(cv, &cfull);
            sc = SlabColor{cv.vol.ptr, cv.vol.pitch, cv.vol.img_pitch, cv.off32};
            hipLaunchKernelGGL((k_raycast_sdf_slab<CELL, true>), grid, dim3(256), 0, (hipStream_t)stream, p, sl, sc);
            return check_launch("kfx_raycast_sdf_slab_color");
        }
    }
    hipLaunchKernelGGL((k_raycast_sdf_slab<CELL, false>), grid, dim3(256), 0, (hipStream_t)stream, p, sl, sc);
    return check_launch("kfx_raycast_sdf_slab");
}

// the dense [9][h w] state of kfx_raycast_sdf_slab as one tile
static SlabRay dense_state(float* state, int init, int w, int h)
{
    SlabRay g{};
    const size_t n = (size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0);
    g.state = state; g.touched = state ? state + 4 * n : nullptr; g.result = state ? state + 5 * n : nullptr; g.P = n; g.R = h > 0 ? h : 1; g.v0 = 0; g.v1 = h; g.fin = nullptr; g.claim_misses = 0;
    g.init = init ? 1 : 0;
    g.adopt_lo = g.adopt_hi = nullptr; g.adopt_tile_major = 0;
    return g;
}

static int raycast_slab_tiles(float* state, float* result, size_t plane_stride, int rows_per_tile, int v0, int v1, int init, int* fin,
                              int claim_misses, const float* adopt_lo, const float* adopt_hi, int layout_flags, const kfx_volume* vol,
                              const kfx_volume* colorvol, const kfx_slab* slab, int own_lo, int own_hi, int w, int h, const float T_wc[12],
                              const float K[4], float near, float far, float trunc_dist, int subpix, kfx_stream stream)
{
    SlabRay g{};
    g.state = state; g.result = result; g.P = plane_stride; g.R = rows_per_tile; g.v0 = v0; g.v1 = v1; g.fin = fin; g.claim_misses = claim_misses ? 1 : 0;
    g.init = init ? 1 : 0;
    const int adopt_tile_major = layout_flags & 1;
    g.adopt_lo = adopt_lo; g.adopt_hi = adopt_hi; g.adopt_tile_major = adopt_tile_major;
    g.packed = (layout_flags & 2) ? 1 : 0;
    g.normals_here = (layout_flags & 4) ? 1 : 0;
    if (g.packed && !(trunc_dist > 0.f)) return set_error(KFX_E_RANGE, "RaycastSdf(slab): the packed tile state needs a positive truncation distance");
    if (((uintptr_t)adopt_lo | (uintptr_t)adopt_hi) & 3) return set_error(KFX_E_ALIGN, "RaycastSdf(slab): alignment of the received snapshots");
    if (!adopt_tile_major && (adopt_lo || adopt_hi) && rows_per_tile > 0 && (v0 / rows_per_tile != (v1 - 1) / rows_per_tile))
        return set_error(KFX_E_SHAPE, "RaycastSdf(slab): one-tile snapshots with rows of several tiles");
    return raycast_slab_launch<RayF32>(g, vol, slab, own_lo, own_hi, w, h, T_wc, K, near, far, trunc_dist, subpix, stream, colorvol);
}

extern "C" int kfx_raycast_sdf_slab_tiles(float* state, float* result, size_t plane_stride, int rows_per_tile, int v0, int v1, int init, int* fin,
                                          int claim_misses, const float* adopt_lo, const float* adopt_hi, int layout_flags, const kfx_volume* vol,
                                          const kfx_slab* slab, int own_lo, int own_hi, int w, int h, const float T_wc[12], const float K[4], float near,
                                          float far, float trunc_dist, int subpix, kfx_stream stream)
{
    return raycast_slab_tiles(state, result, plane_stride, rows_per_tile, v0, v1, init, fin, claim_misses, adopt_lo, adopt_hi, layout_flags, vol, nullptr, slab,
                              own_lo, own_hi, w, h, T_wc, K, near, far, trunc_dist, subpix, stream);
}

// the colour forms (include/kfx_slab_color.h): the same launches with the rank's colour slab
extern "C" int kfx_raycast_sdf_slab_tiles_color(float* state, float* result, size_t plane_stride, int rows_per_tile, int v0, int v1, int init, int* fin,
                                                int claim_misses, const float* adopt_lo, const float* adopt_hi, int layout_flags, const kfx_volume* vol,
                                                const kfx_volume* colorvol, const kfx_slab* slab, int own_lo, int own_hi, int w, int h,
                                                const float T_wc[12], const float K[4], float near, float far, float trunc_dist, int subpix,
                                                kfx_stream stream)
{
    if (!colorvol) return set_error(KFX_E_NULL, "RaycastSdf(slab, colour): null colour volume");
    return raycast_slab_tiles(state, result, plane_stride, rows_per_tile, v0, v1, init, fin, claim_misses, adopt_lo, adopt_hi, layout_flags, vol, colorvol, slab,
                              own_lo, own_hi, w, h, T_wc, K, near, far, trunc_dist, subpix, stream);
}

extern "C" int kfx_raycast_sdf_slab_color(float* state, int init, const kfx_volume* vol, const kfx_volume* colorvol, const kfx_slab* slab, int own_lo,
                                          int own_hi, int w, int h, const float T_wc[12], const float K[4], float near, float far, float trunc_dist,
                                          int subpix, kfx_stream stream)
{
    if (!colorvol) return set_error(KFX_E_NULL, "RaycastSdf(slab, colour): null colour volume");
    return raycast_slab_launch<RayF32>(dense_state(state, init, w, h), vol, slab, own_lo, own_hi, w, h, T_wc, K, near, far, trunc_dist, subpix, stream, colorvol);
}

extern "C" int kfx_raycast_sdf_slab(float* state, int init, const kfx_volume* vol, const kfx_slab* slab, int own_lo, int own_hi,
                                    int w, int h, const float T_wc[12], const float K[4], float near, float far,
                                    float trunc_dist, int subpix, kfx_stream stream)
{
    return raycast_slab_launch<RayF32>(dense_state(state, init, w, h), vol, slab, own_lo, own_hi, w, h, T_wc, K, near, far, trunc_dist, subpix, stream);
}

extern "C" int kfx_raycast_sdf_slab_h(float* state, int init, const kfx_volume* vol, const kfx_slab* slab, int own_lo, int own_hi,
                                      int w, int h, const float T_wc[12], const float K[4], float near, float far,
                                      float trunc_dist, int subpix, kfx_stream stream)
{
    return raycast_slab_launch<RayF16>(dense_state(state, init, w, h), vol, slab, own_lo, own_hi, w, h, T_wc, K, near, far, trunc_dist, subpix, stream);
}

extern "C" int kfx_raycast_state_to_images(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const float* state,
                                           kfx_stream stream)
{
    if (!state) return set_error(KFX_E_NULL, "raycast state: null argument");
    if (int e = check_image(img, 4, 0, 0, "raycast state")) return e;
    if (int e = check_image(depth, 4, cover_w(img), cover_h(img), "raycast state")) return e;
    if (int e = check_image(norm, 16, cover_w(img), cover_h(img), "raycast state")) return e;
    if (img->w == 0 || img->h == 0) return 0;
    RayParams p{};
    p.dptr = (unsigned char*)depth->ptr; p.nptr = (unsigned char*)norm->ptr; p.iptr = (unsigned char*)img->ptr;
    p.dpitch = depth->pitch; p.npitch = norm->pitch; p.ipitch = img->pitch;
    p.w = (int)img->w; p.h = (int)img->h;
    hipLaunchKernelGGL(k_raycast_state_to_images, pixel_grid(p.w, p.h), dim3(256), 0, (hipStream_t)stream, p, state);
    return check_launch("kfx_raycast_state_to_images");
}
