// composite.hip -- the kernels of the multi-GPU raycast composite and their launchers (kfx_composite_*, include/kfx.h): every
// rank ray-casts its own Z-slab; the nearest hit over all slabs wins.  Two collectives carry the data; these kernels pack / select /
// unpack around them, so that a frame costs three small launches instead of a dozen elementwise tensor ops.  The collectives are
// not issued here.  Two drivers order launches and collectives: kfx_slab_composite / kfx_slab_composite_direct (slab.hip) through
// whatever transport stands behind a kfx_comm, and kangaroo_amd/pipeline.py through torch.distributed.  The three images go to the
// kernels as one RenderImages; a pixel's addresses, and what is stored there, through ray_out / write_hit (raycast_ray.h).
//   key     = (depth bits << 8) | rank     positive floats order like their bit patterns; misses = +inf
//   all_reduce(MIN, key)                   -> winner rank and its depth, per pixel
//   payload = winner ? {n.x, n.y, n.z, shade} : 0           all_reduce(SUM, payload)   (n.w = hit ? 1 : 0 comes out of the key)
//
// The direct-send variant (kfx_composite_strips_*): xGMI is a full mesh of point-to-point links, so instead of two ring
// all-reduces over whole images every rank OWNS one strip of the image (pixels [j S, (j + 1) S) of the row-major image,
// S = kfx_composite_strip_pixels):
//   pack:    send[j][c][q] = plane c of pixel j S + q, c = {depth or +inf, n.x, n.y, n.z, shade}    then all-to-all (strip j -> rank j)
//   merge:   of the `world` copies of this rank's strip the nearest depth wins, the lowest rank on ties   then all-gather of the strips
//   unpack:  the merged strips back into the depth / normal / shade images
// 20 bytes per pixel cross each link once in each phase (7/8 of 6.1 MB per rank and phase at 640 x 480 on 8 GPUs, spread over
// seven links at once) against 2 x 7/8 x (2.4 + 4.9) MB in 14 dependent ring steps; same winner per pixel as the key's minimum.
// No reference counterpart (the reference is single-GPU).
#include "kfx_device.h"
#include "host_args.h"
#include "raycast_ray.h"

namespace kfx {

struct CompParams {
    RenderImages im;  // w x h: the launch
    long long* key;   // w*h, dense
    float* payload;   // w*h*4, dense (KFX_COMPOSITE_PAYLOAD floats per pixel)
    int rank;
};

__global__ __launch_bounds__(256) void k_composite_pack(const CompParams p)
{
    int u, v;
    pixel_xy(u, v);
    if (u >= p.im.w || v >= p.im.h) return;
    const float d = *ray_out(p.im, u, v).depth;
    const float dd = isfinite(d) ? d : __builtin_inff();
    p.key[(size_t)v * p.im.w + u] = ((long long)__float_as_uint(dd) << 8) | (long long)p.rank;
}

// after the MIN all-reduce of `key`: keep this rank's normal / shade only where it won
__global__ __launch_bounds__(256) void k_composite_select(const CompParams p)
{
    int u, v;
    pixel_xy(u, v);
    if (u >= p.im.w || v >= p.im.h) return;
    const size_t i = (size_t)v * p.im.w + u;
    const long long k = p.key[i];
    const RayOut o = ray_out(p.im, u, v);
    const float d = *o.depth;
    const bool mine = isfinite(d) && (int)(k & 0xff) == p.rank && (unsigned)(k >> 8) == __float_as_uint(d);
    float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f;
    if (mine) { n = *o.normal; s = *o.shade; }
    reinterpret_cast<float4*>(p.payload)[i] = make_float4(n.x, n.y, n.z, s); // n.w of a hit is 1 (Q8): it travels as the key's hit bit
}

// after the SUM all-reduce of `payload`: write the composite images (depth comes back out of the key).  A miss carries the summed
// payload as it is -- zeros -- with n.w = 0
__global__ __launch_bounds__(256) void k_composite_unpack(const CompParams p)
{
    int u, v;
    pixel_xy(u, v);
    if (u >= p.im.w || v >= p.im.h) return;
    const size_t i = (size_t)v * p.im.w + u;
    const unsigned bits = (unsigned)(p.key[i] >> 8);
    const bool hit = bits < 0x7f800000u;
    const float4 o = reinterpret_cast<const float4*>(p.payload)[i];
    write_hit(ray_out(p.im, u, v), hit ? __uint_as_float(bits) : __builtin_nanf(""), make_float4(o.x, o.y, o.z, hit ? 1.0f : 0.0f), o.w);
}

struct StripParams {
    RenderImages im;
    float* buf;      // strip j: KFX_COMPOSITE_STRIP_PLANES planes of S floats at buf + j * stride
    size_t stride;
    int world;
    unsigned S;
};

__global__ __launch_bounds__(256) void k_strips_pack(const StripParams p)
{
    const unsigned q = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (q >= p.S) return;
    const size_t pix = (size_t)j * p.S + q;
    float d = __builtin_inff();
    float4 n = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f;
    if (pix < (size_t)p.im.w * p.im.h) {
        const int v = (int)(pix / p.im.w), u = (int)(pix - (size_t)v * p.im.w);
        const RayOut in = ray_out(p.im, u, v);
        const float dd = *in.depth;
        if (isfinite(dd)) { d = dd; n = *in.normal; s = *in.shade; }
    }
    float* o = p.buf + (size_t)j * p.stride + q;
    o[0] = d; o[p.S] = n.x; o[2 * (size_t)p.S] = n.y; o[3 * (size_t)p.S] = n.z; o[4 * (size_t)p.S] = s;
}

// in + r * stride: [5][S], rank r's copy of this rank's strip; out: [5][S]
__global__ __launch_bounds__(256) void k_strips_merge(const float* __restrict__ in, float* __restrict__ out, unsigned S, size_t stride, int world)
{
    const unsigned q = blockIdx.x * 256 + threadIdx.x;
    if (q >= S) return;
    unsigned best = 0x7f800000u;   // +inf: no rank hit
    int br = -1;
    for (int r = 0; r < world; ++r) {
        const unsigned b = __float_as_uint(in[(size_t)r * stride + q]);   // depths are positive: they order like their bits
        if (b < best) { best = b; br = r; }
    }
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (br >= 0)
        for (int c = 0; c < 4; ++c) v[c] = in[(size_t)br * stride + (size_t)(1 + c) * S + q];
    out[q] = __uint_as_float(best);
    for (int c = 0; c < 4; ++c) out[(size_t)(1 + c) * S + q] = v[c];
}

// (a miss carries the merged strip's normal and shade as they are -- zeros -- with n.w = 0)
__global__ __launch_bounds__(256) void k_strips_unpack(const StripParams p)
{
    int u, v;
    pixel_xy(u, v);
    if (u >= p.im.w || v >= p.im.h) return;
    const size_t pix = (size_t)v * p.im.w + u;
    const unsigned j = (unsigned)(pix / p.S), q = (unsigned)(pix - (size_t)j * p.S);
    const float* o = p.buf + (size_t)j * p.stride + q;
    const float d = o[0];
    const bool hit = __float_as_uint(d) < 0x7f800000u;
    write_hit(ray_out(p.im, u, v), hit ? d : __builtin_nanf(""), make_float4(o[p.S], o[2 * (size_t)p.S], o[3 * (size_t)p.S], hit ? 1.0f : 0.0f), o[4 * (size_t)p.S]);
}

} // namespace kfx

using namespace kfx;

static int comp_params(CompParams& p, const kfx_image* depth, const kfx_image* norm, const kfx_image* img, long long* key,
                       float* payload, int rank)
{
    if (!key) return set_error(KFX_E_NULL, "composite: null argument");
    if (rank < 0 || rank > 255) return set_error(KFX_E_RANGE, "composite: rank must fit 8 bits");
    if (int e = check_render_images(depth, norm, img, depth, "composite")) return e;
    if (((uintptr_t)key & 7) || ((uintptr_t)payload & 15)) return set_error(KFX_E_ALIGN, "composite: alignment");
    p = CompParams{render_images(depth, norm, img, depth), key, payload, rank};
    return 0;
}

extern "C" int kfx_composite_pack(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, long long* key, int rank, kfx_stream stream)
{
    CompParams p;
    if (int e = comp_params(p, depth, norm, img, key, nullptr, rank)) return e;
    if (p.im.w == 0 || p.im.h == 0) return 0;
    hipLaunchKernelGGL(k_composite_pack, pixel_grid(p.im.w, p.im.h), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_composite_pack");
}

extern "C" int kfx_composite_select(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const long long* key,
                                    float* payload, int rank, kfx_stream stream)
{
    CompParams p;
    if (!payload) return set_error(KFX_E_NULL, "composite: null payload");
    if (int e = comp_params(p, depth, norm, img, const_cast<long long*>(key), payload, rank)) return e;
    if (p.im.w == 0 || p.im.h == 0) return 0;
    hipLaunchKernelGGL(k_composite_select, pixel_grid(p.im.w, p.im.h), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_composite_select");
}

extern "C" int kfx_composite_unpack(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const long long* key,
                                    const float* payload, kfx_stream stream)
{
    CompParams p;
    if (!payload) return set_error(KFX_E_NULL, "composite: null payload");
    if (int e = comp_params(p, depth, norm, img, const_cast<long long*>(key), const_cast<float*>(payload), 0)) return e;
    if (p.im.w == 0 || p.im.h == 0) return 0;
    hipLaunchKernelGGL(k_composite_unpack, pixel_grid(p.im.w, p.im.h), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_composite_unpack");
}

// ---- direct-send variant ----
extern "C" size_t kfx_composite_strip_pixels(size_t w, size_t h, int world)
{
    if (world < 1) return 0;
    const size_t per = (w * h + (size_t)world - 1) / (size_t)world;
    return (per + 63) / 64 * 64;   // 256-byte planes
}

static int strip_params(StripParams& p, const kfx_image* depth, const kfx_image* norm, const kfx_image* img, float* buf, size_t stride, int world)
{
    if (!buf) return set_error(KFX_E_NULL, "composite strips: null argument");
    if (world < 1 || world > 256) return set_error(KFX_E_RANGE, "composite strips: world in [1, 256]");
    if (int e = check_render_images(depth, norm, img, depth, "composite strips")) return e;
    if ((uintptr_t)buf & 3) return set_error(KFX_E_ALIGN, "composite strips: alignment");
    const size_t S = kfx_composite_strip_pixels(depth->w, depth->h, world);
    if (S > 0x7fffffffull) return set_error(KFX_E_RANGE, "composite strips: image too large");
    if (stride && stride < KFX_COMPOSITE_STRIP_PLANES * S) return set_error(KFX_E_SHAPE, "composite strips: rank stride smaller than a strip");
    p = StripParams{render_images(depth, norm, img, depth), buf, stride ? stride : KFX_COMPOSITE_STRIP_PLANES * S, world, (unsigned)S};
    return 0;
}

extern "C" int kfx_composite_strips_pack(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, float* send, size_t rank_stride, int world,
                                         kfx_stream stream)
{
    StripParams p;
    if (int e = strip_params(p, depth, norm, img, send, rank_stride, world)) return e;
    if (p.S == 0) return 0;
    hipLaunchKernelGGL(k_strips_pack, dim3(ceil_div(p.S, 256u), world), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_composite_strips_pack");
}

extern "C" int kfx_composite_strips_merge(const float* recv, float* merged, size_t strip_pixels, size_t rank_stride, int world, kfx_stream stream)
{
    if (!recv || !merged) return set_error(KFX_E_NULL, "kfx_composite_strips_merge: null argument");
    if (world < 1 || world > 256 || strip_pixels > 0x7fffffffull) return set_error(KFX_E_RANGE, "kfx_composite_strips_merge: world / strip size");
    if (((uintptr_t)recv | (uintptr_t)merged) & 3) return set_error(KFX_E_ALIGN, "kfx_composite_strips_merge: alignment");
    if (rank_stride && rank_stride < KFX_COMPOSITE_STRIP_PLANES * strip_pixels) return set_error(KFX_E_SHAPE, "kfx_composite_strips_merge: rank stride smaller than a strip");
    if (strip_pixels == 0) return 0;
    hipLaunchKernelGGL(k_strips_merge, dim3(ceil_div((unsigned)strip_pixels, 256u)), dim3(256), 0, (hipStream_t)stream, recv, merged, (unsigned)strip_pixels,
                       rank_stride ? rank_stride : KFX_COMPOSITE_STRIP_PLANES * strip_pixels, world);
    return check_launch("kfx_composite_strips_merge");
}

extern "C" int kfx_composite_strips_unpack(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const float* strips, size_t rank_stride,
                                           int world, kfx_stream stream)
{
    StripParams p;
    if (int e = strip_params(p, depth, norm, img, const_cast<float*>(strips), rank_stride, world)) return e;
    if (p.im.w == 0 || p.im.h == 0) return 0;
    hipLaunchKernelGGL(k_strips_unpack, pixel_grid(p.im.w, p.im.h), dim3(256), 0, (hipStream_t)stream, p);
    return check_launch("kfx_composite_strips_unpack");
}
