// raycast_ray.h -- the ray of RaycastSdf (src/cu_raycast.cu:14-113), written once for every renderer that marches one: the dense
// marches of raycast.hip and the march over packed bricks of raycast_bricks.hip (analytic.hip takes the shade).  The parameter block
// and its host-side fill, the pixel a lane carries and the launch's tiling, the ray and its slab test against the box, the plain
// march loop over any sampler, and what a ray writes -- the hit epilogue over whatever source the gradient and the colour sample come from.
#pragma once

#include <type_traits>

#include "kfx_device.h"
#include "sampling.h"

namespace kfx {

struct RayParams {
    VolView vol;
    V3 size;          // bbox.Size()
    V3 dims1;         // (w-1.f, h-1.f, d-1.f)           Volume.h:226
    V3 hi2;           // ((float)(w-2), (float)(h-2), (float)(d-2))   Volume.h:229-231
    V3 voxel;         // VoxelSizeUnits()                BoundedVolume.h:67-76
    V3 inv_size;      // 1 / size, for div_uniform
    int fastdiv, off32;
    Pose T;           // T_wc
    Intr K;
    unsigned char *dptr, *nptr, *iptr;
    size_t dpitch, npitch, ipitch;
    int w, h;
    float near, far, trunc;
    int subpix;
    int tile_log2w;   // log2 of the wave's pixel-tile width (3: 8x8, 4: 16x4, 5: 32x2)
    int wg_log2x;     // log2 of the number of wave tiles side by side in a workgroup (0: 1x4, 1: 2x2, 2: 4x1)
    int sparse_lanes; // 0, or the number of lanes per wave that carry rays (small images; KFX_RAYCAST_LANES = 8 / 16 / 32 forces it, -1 disables it)
};

// PhongShade (cu_raycast.cu:14-28)
__device__ __forceinline__ float phong(const V3 p_c, const V3 n_c)
{
    const float ambient = (float)0.4, diffuse = (float)0.4, specular = (float)0.2;
    const V3 eyedir = div_s(p_c * -1.0f, length(p_c));
    const V3 l0 = v3((float)0.4, (float)0.4, -1.0f);
    const V3 lightdir = div_s(l0, length(l0));
    const float ldotn = dot(lightdir, n_c);
    const V3 lightreflect = n_c * (2 * ldotn) + lightdir * -1.0f;
    const float edotr = fmaxf(0.0f, dot(eyedir, lightreflect));
    const float spec = edotr * edotr * edotr * edotr * edotr * edotr * edotr * edotr * edotr * edotr;
    return ambient + diffuse * ldotn + specular * spec;
}

// pixel of thread `tid` of workgroup (bx, by): wave -> (1 << tile_log2w) x (64 >> tile_log2w) pixel tile,
// workgroup -> 2 x 2 such tiles (wg_log2x = 1)
__device__ __forceinline__ void ray_pixel_of(const RayParams& p, int bx, int by, int tid, int& u, int& v)
{
    const int lane = tid & 63, wv = tid >> 6;
    const int tw = 1 << p.tile_log2w, th = 64 >> p.tile_log2w;
    const int wgx = 1 << p.wg_log2x, wgy = 4 >> p.wg_log2x; // waves per workgroup along x / y
    u = (bx * wgx + (wv & (wgx - 1))) * tw + (lane & (tw - 1));
    v = (by * wgy + (wv >> p.wg_log2x)) * th + (lane >> p.tile_log2w);
}

// The same for a launch with sparse lanes (sparse != 0: small images and coarse pyramid levels).  Only the first `sparse` lanes
// of a wave carry rays, a strip of one pixel row, and a workgroup is 2 x 2 strips: neighbouring rays are many voxels apart
// there, so every lane of a load fetches its own line and a wave-step waits for the slowest of its misses -- of `sparse`
// instead of 64.  Returns whether the lane carries a ray.
__device__ __forceinline__ bool ray_lane_pixel(const RayParams& p, int sparse, int bx, int by, int& u, int& v)
{
    if (!sparse) {
        ray_pixel_of(p, bx, by, threadIdx.x, u, v);
        return true;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    u = (bx * 2 + (wv & 1)) * sparse + lane;
    v = by * 2 + (wv >> 1);
    return lane < sparse;
}

// The ray of pixel (u, v) and the slab test against the volume's box (cu_raycast.cu:40-51): the one definition the marches, the
// workgroups' vote before their prologue (k_raycast_sdf_classes) and the epilogue (write_ray: the ray alone) share.
struct RayBox { V3 c_w, ray_c, ray_w; float max_tmin, min_tmax; };
__device__ __forceinline__ RayBox ray_box(const RayParams& p, const int u, const int v)
{
    RayBox b;
    b.c_w = v3(p.T.m[3], p.T.m[7], p.T.m[11]);                                        // SE3Translation
    b.ray_c = v3(((float)u - p.K.u0) / p.K.fu, ((float)v - p.K.v0) / p.K.fv, 1.0f);   // Unproject
    b.ray_w = so3_mul(p.T, b.ray_c);
    const V3 ta = div_cw(p.vol.bmin - b.c_w, b.ray_w);
    const V3 tb = div_cw(p.vol.bmax - b.c_w, b.ray_w);
    const V3 tmin = v3(fminf(ta.x, tb.x), fminf(ta.y, tb.y), fminf(ta.z, tb.z));
    const V3 tmax = v3(fmaxf(ta.x, tb.x), fmaxf(ta.y, tb.y), fmaxf(ta.z, tb.z));
    b.max_tmin = fmaxf(fmaxf(fmaxf(tmin.x, tmin.y), tmin.z), p.near);
    b.min_tmax = fminf(fminf(fminf(tmax.x, tmax.y), tmax.z), p.far);
    return b;
}
__device__ __forceinline__ bool enters(const RayBox& b) { return b.max_tmin < b.min_tmax; }

// the surface normal in the camera frame (cu_raycast.cu:92-97) from the gradient g: normalised, (0, 0, 1) where it vanishes
__device__ __forceinline__ V3 normal_of(const Pose& T, const V3 g)
{
    const float len = length(g);
    const V3 n_w = len > 0 ? div_s(g, len) : v3(0.f, 0.f, 1.f);
    return so3_mul_inv(T, n_w);
}
// ... at pos_w of a dense volume
template <typename CELL>
__device__ __forceinline__ V3 normal_c(const RayParams& p, const V3 pos_w)
{
    return normal_of(p.T, gradient<CELL>(p, pos_w));
}

// where pixel (u, v) of the three output images lies; p: a RayParams, or a RenderImages (kfx_device.h) -- the same eight members
struct RayOut { float* depth; float* shade; float4* normal; };
template <typename IMAGES>
__device__ __forceinline__ RayOut ray_out(const IMAGES& p, const int u, const int v)
{
    return RayOut{reinterpret_cast<float*>(p.dptr + (size_t)v * p.dpitch) + u, reinterpret_cast<float*>(p.iptr + (size_t)v * p.ipitch) + u,
                  reinterpret_cast<float4*>(p.nptr + (size_t)v * p.npitch) + u};
}
// what a ray that hits nothing writes (cu_raycast.cu:104-108)
__device__ __forceinline__ void write_no_hit(const RayOut& o)
{
    *o.depth = __builtin_nanf("");
    *o.shade = 0.f;
    *o.normal = make_float4(0.f, 0.f, 0.f, 0.f);
}
// ... and a pixel that has something to show: the caller's values as they are (normal.w = 1 marks a hit: cu_raycast.cu:101)
__device__ __forceinline__ void write_hit(const RayOut& o, const float depth, const float4 normal, const float shade)
{
    *o.depth = depth;
    *o.shade = shade;
    *o.normal = normal;
}

// The plain march of a ray that enters the box (cu_raycast.cu:58-88) over any sampler, float sample(p, pos_w) -- p a RayParams or a
// block derived from it, handed through to the sampler: steps of max(sdf, min_delta) -- trunc for a NaN sample -- from the box's near
// side until a sample at or behind a surface; a hit where the sample before it was positive, refined between the two with subpix.
// Returns the hit's depth along the ray, 0 without one.  (The slab march and the class-table march of raycast.hip keep loops of
// their own: theirs carry a hand-over between ranks and the tables' runs through the same steps.)
template <typename PARAMS, typename SAMPLE>
__device__ __forceinline__ float march_plain(const PARAMS& p, const RayBox& box, const SAMPLE& sample)
{
    const V3 c_w = box.c_w, ray_w = box.ray_w;
    const float max_tmin = box.max_tmin, min_tmax = box.min_tmax;
    float depth = 0.0f;
    float lambda = max_tmin;
    float last_sdf = __builtin_nanf("");
    const float min_delta = p.voxel.x;
    float delta = 0.f;
    while (lambda < min_tmax) {
        const float sdf = sample(p, c_w + ray_w * lambda);
        if (sdf <= 0) {
            if (last_sdf > 0) {
                if (p.subpix) lambda = lambda + delta * sdf / (last_sdf - sdf);
                depth = lambda;
            }
            break;
        }
        delta = march_step(sdf, min_delta, p.trunc);
        lambda += delta;
        last_sdf = sdf;
    }
    return depth;
}

// What a ray writes (cu_raycast.cu:90-108): depth, normal and shade of a hit at `depth` along the ray (depth > 0), else "no
// hit".  q is the parameter block to read from: the kernel's arguments, or the class kernels' copy of them in LDS -- the ray
// again, the same expressions on the same values.  gradient_at(pos_w) is the SDF's gradient there -- gradient<CELL> on a dense
// volume, gradient_over on a brick accessor --; shade is PhongShade{}, or a float shade(pos_w) for the colour variant: img =
// colorVol.GetUnitsTrilinearClamped(pos_w) instead of the Phong shade (cu_raycast.cu:172,179).
struct PhongShade {};
template <typename GRADIENT, typename SHADE>
__device__ __forceinline__ void write_ray(const RayParams& q, const int u, const int v, const float depth, const GRADIENT& gradient_at, const SHADE& shade)
{
    const RayOut o = ray_out(q, u, v);
    if (depth > 0) {
        const RayBox r = ray_box(q, u, v);
        const V3 n_c = normal_of(q.T, gradient_at(r.c_w + r.ray_w * depth));
        *o.depth = depth;   // (write_hit's stores, the depth ahead of the shade's arithmetic: the order the march kernels were scheduled with)
        if constexpr (std::is_same<SHADE, PhongShade>::value) *o.shade = phong(r.ray_c * depth, n_c);
        else *o.shade = shade(r.c_w + r.ray_w * depth);
        *o.normal = make_float4(n_c.x, n_c.y, n_c.z, 1.0f);
    } else {
        write_no_hit(o);
    }
}

// Host side: the members of a RayParams that do not describe the volume -- pose, intrinsics, the three images, the launch's size
// (the reference bounds it by img, cu_raycast.cu:39,110), the march's parameters, the default tiling.  After the caller's checks.
inline void ray_fill(RayParams& p, const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const float T_wc[12], const float K[4],
                     float near, float far, float trunc_dist, int subpix)
{
    for (int i = 0; i < 12; ++i) p.T.m[i] = T_wc[i];
    p.K = Intr{K[0], K[1], K[2], K[3]};
    p.dptr = (unsigned char*)depth->ptr;
    p.nptr = (unsigned char*)norm->ptr;
    p.iptr = (unsigned char*)img->ptr;
    p.dpitch = depth->pitch;
    p.npitch = norm->pitch;
    p.ipitch = img->pitch;
    p.w = (int)img->w;
    p.h = (int)img->h;
    p.near = near;
    p.far = far;
    p.trunc = trunc_dist;
    p.subpix = subpix ? 1 : 0;
    p.tile_log2w = 5; // 32 x 2 pixel wave tiles, 2 x 2 of them per workgroup
    p.wg_log2x = 1;
    p.sparse_lanes = 0;
}

// Host side: the pixel tiling of a launch of p.w x p.h rays (both positive) under the knobs KFX_RAYCAST_TILE / _WG / _LANES, each read
// once per process: sets p's mapping and returns the grid of 256-thread workgroups.
inline dim3 ray_tiling(RayParams& p)
{
    static const int tile_env = env_int("KFX_RAYCAST_TILE", 5, 0, 6);
    static const int wg_env = env_int("KFX_RAYCAST_WG", 1, 0, 2);
    static const int lanes_env = [] { const int v = env_int("KFX_RAYCAST_LANES", 0); return (v == 8 || v == 16 || v == 32) ? v : (v < 0 ? -1 : 0); }();
    p.tile_log2w = tile_env;
    p.wg_log2x = wg_env;
    // small images (pyramid levels): rays of a wave are many voxels apart, 16 rays per wave wait for fewer misses per step
    const int lanes = lanes_env ? lanes_env : ((long long)p.w * p.h <= 160 * 120 ? 16 : 0);
    if (lanes && lanes_env >= 0) {
        p.sparse_lanes = lanes;
        return dim3(ceil_div(p.w, 2 * lanes), ceil_div(p.h, 2));
    }
    return dim3(ceil_div(p.w, (1 << p.wg_log2x) << p.tile_log2w), ceil_div(p.h, (4 >> p.wg_log2x) * (64 >> p.tile_log2w)));
}

} // namespace kfx
