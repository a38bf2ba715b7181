// host_args.h -- what the launchers decide alike on the host: what a usable kfx_volume and a usable kfx_image are, the grid of a
// per-pixel launch, how a Z-slab is seen through the whole volume's geometry, how a process-wide knob is read, how a sequence of
// steps that must all be entered keeps its first error.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kfx_device.h"

namespace kfx {

// dimensions end at 65535 where kernels keep cell coordinates in 16 bits; operators without that limit pass VOLUME_ANY_DIM
constexpr size_t VOLUME_MAX_DIM = 65535, VOLUME_ANY_DIM = ~(size_t)0;

// A usable volume of cell_bytes-byte cells: non-null, every dimension in [min_dim, max_dim], a row / a slice within its pitch,
// pointer and pitches aligned to the cell -- in that order at every entry point.  `what` names the operator in the message.
// "<what>: <rule>" as the last error
inline int fail_rule(const char* what, int code, const char* rule)
{
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", what, rule);
    return set_error(code, msg);
}
// the verdict {code, rule} of a host-side rule (bricks_host.h: BrickRefusal) as the entry point's answer: 0 where it accepted
template <typename REFUSAL>
inline int refuse(const REFUSAL& r, const char* what) { return r.code ? fail_rule(what, r.code, r.rule) : 0; }

inline int check_volume(const kfx_volume* vol, size_t cell_bytes, size_t min_dim, size_t max_dim, const char* what)
{
    auto fail = [what](int code, const char* rule) { return fail_rule(what, code, rule); };
    if (!vol || !vol->ptr) return fail(KFX_E_NULL, "null volume");
    if (vol->w < min_dim || vol->h < min_dim || vol->d < min_dim || vol->w > max_dim || vol->h > max_dim || vol->d > max_dim)
        return fail(KFX_E_SHAPE, "volume dimensions");
    if (vol->pitch < vol->w * cell_bytes || vol->img_pitch < vol->pitch * (vol->h - 1) + vol->w * cell_bytes)
        return fail(KFX_E_SHAPE, "volume pitch smaller than a row / slice");
    if (((uintptr_t)vol->ptr | vol->pitch | vol->img_pitch) & (cell_bytes - 1)) return fail(KFX_E_ALIGN, "volume not aligned to its cell size");
    return 0;
}

// A usable image of elem-byte pixels that covers min_w x min_h (the consumer's launch; 0, 0: any size): non-null; at least that
// large, a row of its OWN w pixels within its pitch (rows of a usable view do not overlap), no dimension above 2^30 (kernels keep
// pixel coordinates in int); pointer and pitch aligned to the largest power of two in elem, 16 at the most (3-byte RGB: bytes,
// float4: 16) -- in that order at every entry point.  `what` names the operator and the image in the message.
inline int check_image(const kfx_image* im, size_t elem, size_t min_w, size_t min_h, const char* what)
{
    if (!im || !im->ptr) return fail_rule(what, KFX_E_NULL, "null image");
    if (im->w < min_w || im->h < min_h) return fail_rule(what, KFX_E_SHAPE, "image smaller than the launch");
    if (im->pitch < im->w * elem) return fail_rule(what, KFX_E_SHAPE, "image pitch smaller than a row");
    if (im->w > (1u << 30) || im->h > (1u << 30)) return fail_rule(what, KFX_E_SHAPE, "image dimensions above 2^30");
    const size_t pow2 = elem & (~elem + 1), al = pow2 < 16 ? pow2 : 16;
    if (((uintptr_t)im->ptr | im->pitch) & (al - 1)) return fail_rule(what, KFX_E_ALIGN, "image not aligned to its pixel size");
    return 0;
}

// the device's view of a usable image
inline ImgView img_view(const kfx_image& im) { return ImgView{(const unsigned char*)im.ptr, im.pitch, (int)im.w, (int)im.h}; }

// What the input of a launch bounded by `out` has to cover where the entry point answers an empty launch with 0 before it compares
// sizes: nothing then.
inline size_t cover_w(const kfx_image* out) { return out->h ? out->w : 0; }
inline size_t cover_h(const kfx_image* out) { return out->w ? out->h : 0; }

// The rendering trio -- depth (float), normals (float4), shading image (float) -- each covering `lead`, the one of the three that
// bounds the launch (RaycastSdf: img, as the reference; the composite: depth).
inline int check_render_images(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const kfx_image* lead, const char* what)
{
    if (!lead) return fail_rule(what, KFX_E_NULL, "null image");
    if (int e = check_image(depth, 4, lead->w, lead->h, what)) return e;
    if (int e = check_image(norm, 16, lead->w, lead->h, what)) return e;
    return check_image(img, 4, lead->w, lead->h, what);
}

// the device's view of a usable rendering trio; `lead` bounds the launch
inline RenderImages render_images(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const kfx_image* lead)
{
    return RenderImages{(unsigned char*)depth->ptr, (unsigned char*)norm->ptr, (unsigned char*)img->ptr, depth->pitch, norm->pitch, img->pitch, (int)lead->w, (int)lead->h};
}

// the grid of a per-pixel launch: workgroups of 256 = PIX_W x PIX_H pixels, whose threads find their pixel with pixel_xy (kfx_device.h)
inline dim3 pixel_grid(int w, int h) { return dim3(ceil_div(w, PIX_W), ceil_div(h, PIX_H)); }

// The packed texel image of a w x h depth image (kfx_device.h: texel_put / texel_block_max write it, the tiled SdfFuse kernels stage it by LDS-DMA):
// texel rows of tpitch bytes -- w * 16 rounded up to 256 -- then the maxima of the 8 x 4 pixel blocks, bh4 rows of bw8 floats
struct TexLayout { size_t tpitch, bmax_off, bytes; unsigned bw8, bh4; };
inline TexLayout tex_layout(size_t w, size_t h)
{
    TexLayout t;
    t.tpitch = (w * 16 + 255) / 256 * 256;
    t.bw8 = (unsigned)((w + 63) / 64 * 8);
    t.bh4 = (unsigned)((h + 3) / 4);
    t.bmax_off = t.tpitch * h;
    t.bytes = t.bmax_off + (size_t)t.bw8 * t.bh4 * sizeof(float);
    return t;
}

// The full volume a Z-slab (planes [z_offset, z_offset + d) of full_d) belongs to, for set_geometry / set_voxel_size: the base
// pointer moved back by z_offset planes -- a virtual base, dereferenced only inside the stored planes -- and the full extent in z.
inline kfx_volume slab_full_volume(const kfx_volume* vol, const kfx_slab* slab)
{
    kfx_volume full = *vol;
    full.ptr = (unsigned char*)vol->ptr - (ptrdiff_t)slab->z_offset * (ptrdiff_t)vol->img_pitch;
    full.d = slab->full_d;
    full.boxmin[2] = slab->full_zmin;
    full.boxmax[2] = slab->full_zmax;
    return full;
}

// A rank's colour slab beside its SDF slab (include/kfx_slab_color.h): the colour volume is partitioned exactly like the SDF volume,
// so the two local views have the same dimensions and the same box.  Both volumes non-null (the callers have checked).
inline int check_color_slab(const kfx_volume* vol, const kfx_volume* colorvol, const char* what)
{
    char msg[200];
    if (colorvol->w != vol->w || colorvol->h != vol->h || colorvol->d != vol->d) {
        snprintf(msg, sizeof(msg), "%s: the colour slab's dimensions differ from the SDF slab's", what);
        return set_error(KFX_E_SHAPE, msg);
    }
    for (int i = 0; i < 3; ++i)
        if (memcmp(&colorvol->boxmin[i], &vol->boxmin[i], sizeof(float)) != 0 || memcmp(&colorvol->boxmax[i], &vol->boxmax[i], sizeof(float)) != 0) {
            snprintf(msg, sizeof(msg), "%s: the colour slab's box differs from the SDF slab's", what);
            return set_error(KFX_E_SHAPE, msg);
        }
    return 0;
}

// A numeric knob of the environment (clamped to [lo, hi]); callers keep it in a function-local static: read once, at first use.
inline int env_int(const char* name, int dflt)
{
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
inline int env_int(const char* name, int dflt, int lo, int hi)
{
    const int v = env_int(name, dflt);
    return v < lo ? lo : (v > hi ? hi : v);
}
inline float env_float(const char* name, float dflt)
{
    const char* e = getenv(name);
    return e ? (float)atof(e) : dflt;
}
// whether the knob is set to something that begins with `prefix`
inline bool env_begins(const char* name, const char* prefix)
{
    const char* e = getenv(name);
    return e && strncmp(e, prefix, strlen(prefix)) == 0;
}

// "First error wins, go on regardless": a rank must not skip a collective its peers enter (they would wait for ever), so a step's
// failure is noted, the steps after it are entered all the same, and the first error is what the caller returns at the end.
struct FirstError {
    int status = 0;
    void operator()(int e) { if (e && !status) status = e; }
};

} // namespace kfx
