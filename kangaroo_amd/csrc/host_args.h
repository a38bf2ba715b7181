// host_args.h -- what the launchers decide alike on the host: what a usable kfx_volume is, how a Z-slab is seen through the
// whole volume's geometry, how a process-wide knob is read.
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
inline int check_volume(const kfx_volume* vol, size_t cell_bytes, size_t min_dim, size_t max_dim, const char* what)
{
    auto fail = [what](int code, const char* rule) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: %s", what, rule);
        return set_error(code, msg);
    };
    if (!vol || !vol->ptr) return fail(KFX_E_NULL, "null volume");
    if (vol->w < min_dim || vol->h < min_dim || vol->d < min_dim || vol->w > max_dim || vol->h > max_dim || vol->d > max_dim)
        return fail(KFX_E_SHAPE, "volume dimensions");
    if (vol->pitch < vol->w * cell_bytes || vol->img_pitch < vol->pitch * (vol->h - 1) + vol->w * cell_bytes)
        return fail(KFX_E_SHAPE, "volume pitch smaller than a row / slice");
    if (((uintptr_t)vol->ptr | vol->pitch | vol->img_pitch) & (cell_bytes - 1)) return fail(KFX_E_ALIGN, "volume not aligned to its cell size");
    return 0;
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

} // namespace kfx
