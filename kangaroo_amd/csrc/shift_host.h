// shift_host.h -- the plan of kfx_volume_shift (include/kfx_shift.h) and the box of the shifted volume: what shift.hip decides on the
// host before it launches anything.  No HIP in here: scripts/shift_host_check.cpp drives it under the host sanitizers, and
// kfx_volume_shift_plan returns its list so that the hazard argument can be checked without a device.
#pragma once

#include <stddef.h>

#include "../../include/kfx_shift.h"

namespace kfx {

inline size_t shift_cell_bytes(int cell) { return cell == KFX_CELL_F32 ? 8 : ((cell == KFX_CELL_F16 || cell == KFX_CELL_COLOR) ? 4 : 0); }

struct ShiftGeom {
    int w, h, d;              // cells of the view
    int sx, sy, sz;
    size_t plane_bytes;       // one packed z-plane: w * h * cell bytes
};

inline bool shift_is_zero(const ShiftGeom& g) { return g.sx == 0 && g.sy == 0 && g.sz == 0; }
// no cell has its source inside the view: the whole shift is one fill
inline bool shift_is_fill(const ShiftGeom& g)
{
    const auto out = [](long long s, long long n) { return s >= n || -s >= n; };
    return out(g.sx, g.w) || out(g.sy, g.h) || out(g.sz, g.d);
}
// chunks are staged through the scratch: an in-plane shift, whose source and destination planes are the same
inline bool shift_is_staged(const ShiftGeom& g) { return !shift_is_zero(g) && !shift_is_fill(g) && g.sz == 0; }
// one packed plane, rounded up to 256 bytes; 0 where the plan has no STAGE
inline size_t shift_min_scratch(const ShiftGeom& g) { return shift_is_staged(g) ? (g.plane_bytes + 255) / 256 * 256 : 0; }

// The launches of a shift, in stream order, each handed to emit(kfx_shift_step); returns their number.  scratch_planes: the packed
// planes the caller's scratch holds (>= 1 where the plan stages).
//   sz != 0: DIRECT chunks of P = |sz| planes over the planes that have a source -- [0, d - sz) ascending for sz > 0, [-sz, d)
//            descending for sz < 0 -- then one FILL of the |sz| planes that have none.  A chunk reads planes [z0 + sz, z1 + sz): |sz| >= P
//            away from those it writes, and the planes it overwrites were the sources of this or an earlier chunk.  The FILL comes
//            last because its planes are the sources of the last chunks.
//   sz == 0: STAGE + PLACE per chunk of P = min(scratch_planes, d) planes, ascending.
template <typename Emit>
inline int shift_plan(const ShiftGeom& g, size_t scratch_planes, Emit emit)
{
    int n = 0;
    const auto step = [&](int kind, int d0, int d1, int s0, int s1) { emit(kfx_shift_step{kind, d0, d1, s0, s1}); ++n; };
    if (shift_is_zero(g)) return 0;
    if (shift_is_fill(g)) { step(KFX_SHIFT_FILL, 0, g.d, 0, 0); return n; }
    if (g.sz > 0) {
        const int P = g.sz, end = g.d - g.sz;
        for (int z0 = 0; z0 < end; z0 += P) {
            const int z1 = z0 + P < end ? z0 + P : end;
            step(KFX_SHIFT_DIRECT, z0, z1, z0 + g.sz, z1 + g.sz);
        }
        step(KFX_SHIFT_FILL, end, g.d, 0, 0);
    } else if (g.sz < 0) {
        const int P = -g.sz, begin = -g.sz;
        for (int z1 = g.d; z1 > begin; z1 -= P) {
            const int z0 = z1 - P > begin ? z1 - P : begin;
            step(KFX_SHIFT_DIRECT, z0, z1, z0 + g.sz, z1 + g.sz);
        }
        step(KFX_SHIFT_FILL, 0, begin, 0, 0);
    } else {
        const int P = scratch_planes < (size_t)g.d ? (int)scratch_planes : g.d;
        if (P < 1) return 0;   // (callers refuse a scratch below the minimum before they get here)
        for (int z0 = 0; z0 < g.d; z0 += P) {
            const int z1 = z0 + P < g.d ? z0 + P : g.d;
            step(KFX_SHIFT_STAGE, 0, z1 - z0, z0, z1);
            step(KFX_SHIFT_PLACE, z0, z1, 0, z1 - z0);
        }
    }
    return n;
}

// BoundedVolume::VoxelPositionInUnits of one axis: min + size * i / (float)(dim - 1), every operation rounded to fp32 (the
// translation units that include this are compiled without contraction)
inline float shift_voxel_position(float bmin, float bmax, long long i, size_t dim)
{
    const float size = bmax - bmin;
    const float num = size * (float)i;
    const float q = num / (float)(dim - 1);
    return bmin + q;
}

inline void shift_box(const kfx_volume& v, const int shift[3], float bmin[3], float bmax[3])
{
    const size_t dims[3] = {v.w, v.h, v.d};
    for (int a = 0; a < 3; ++a) {
        bmin[a] = shift_voxel_position(v.boxmin[a], v.boxmax[a], shift[a], dims[a]);
        bmax[a] = shift_voxel_position(v.boxmin[a], v.boxmax[a], (long long)dims[a] - 1 + shift[a], dims[a]);
    }
}

// what kfx_frame_shift (shift.hip) needs of a kfx_frame (frame.hip): its volume, whose box a shift moves, and the summary to rebuild
// when the frame tracks (else null)
kfx_volume* frame_volume(kfx_frame* f);
kfx_sdf_summary* frame_tracked_summary(kfx_frame* f);

// the fill cell's bytes (shift.hip): {fill, 0} as SDF_t, the half of fill and a zero weight as SDF_h, fill itself as a colour cell (the
// 4-byte cells: the low word).  bricks.hip compares against the same bytes.
unsigned long long shift_fill_bytes(int cell, float fill);

} // namespace kfx
