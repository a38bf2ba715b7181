/* kfx_summary_h.h -- the brick summary of include/kfx.h (kfx_sdf_summary) for half-cell volumes: the _h counterparts of its
 * tracked entry points.  Same library (libkfx.so); kept out of kfx.h, whose declarations are the fp32 path. */
#ifndef KFX_SUMMARY_H_H
#define KFX_SUMMARY_H_H

#include "kfx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the brick summary of a half-cell volume (roo::SDF_h, BASELINE config C5) ------------------------------------------
 * kfx_sdf_summary_create_h makes a summary of a BoundedVolume<SDF_h>; it takes the _h calls below, and kfx_sdf_summary_invalidate /
 * _rebuild / _destroy.  A half summary passed to a call of the fp32 block above, or an fp32 summary to the _h calls, is
 * rejected with KFX_E_SHAPE before anything is launched.  Tracking only observes: the volume is bit-identical to kfx_sdf_fuse_h's.
 *   vref: the value of class 1 is trunc_dist ROUNDED TO HALF -- what an untouched free cell holds and the plain half march samples
 *     (kfx_sdf_reset_tracked_h records that value); the step through such an entry is max(vref, voxel size).  Class 3 ("vref or
 *     NaN") is crossed only where that step equals trunc_dist, i.e. where trunc_dist is itself a half value.
 *   exact numerics: only cells bit-equal to vref (or NaN) qualify -- images bit-identical to kfx_raycast_sdf_h.  A free cell holds
 *     vref after its first observation only (the half running average of the second one rounds away from it), so on a running
 *     stream mostly never-observed space qualifies and the quarter rule picks the plain march: correct, not a defect.
 *   fast numerics: cells within KFX_SUMMARY_HALF_BAND (relative) of vref.  The half running average keeps the reference's
 *     operation order, every intermediate rounded to half, and with the real per-voxel weights observed free space does a random
 *     walk around vref that widens with the frames: at most 1.2 % after 60 frames, 7.9 % after 600 (S_room / S_full at 64^3,
 *     scripts/half_free_band.py with the CPU oracle's half fuse; profiles/r07_c5_tables/half_free_band.json).  The band covers
 *     600 frames with a margin of 1.6; on longer streams free cells leave class 1 one by one (less skipping, still correct).
 *     A band that wide admits cells just inside the truncation band in front of a surface, so after a class-1 run the crossing
 *     sample's predecessor is sampled (as after class 3) instead of being taken as vref.  Depth within the fast-mode tolerance
 *     of the exact march.
 * Global-table mode (fp32 and half): where the class tables with the levels derived from them exceed the LDS budget (a parent
 * volume of ~2000^3 cells or more), or with KFX_RAYCAST_GLOBAL_TABLES=1, the table build uses a 16^3-cell fine level and also
 * writes the 64^3- and 128^3-cell levels to global memory; the march stages only those two (d_counters[5] of the count calls
 * reports their bytes) and looks up the 32^3-cell and fine levels in global memory, coarse level first -- the same skips, the
 * same images.  kfx_raycast_sdf_levels_tracked[_h] run the plain levels march in this mode. */
#define KFX_SUMMARY_HALF_BAND 0.125f   /* 2^-3 relative to vref: fast-numerics tolerance of half cells (fp32 cells: 1e-5) */
int kfx_sdf_summary_create_h(kfx_sdf_summary** out, const kfx_volume* vol);
int kfx_sdf_reset_tracked_h(const kfx_volume* vol, kfx_sdf_summary* s, float trunc_dist, kfx_stream stream);
int kfx_sdf_fuse_tracked_h(const kfx_volume* vol, kfx_sdf_summary* s, const kfx_image* depth, const kfx_image* norm,
                           const float T_cw[12], const float K[4], float trunc_dist, float max_w, float mincostheta,
                           unsigned flags, kfx_stream stream);
int kfx_raycast_sdf_tracked_h(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const kfx_volume* vol,
                              kfx_sdf_summary* s, const float T_wc[12], const float K[4], float near, float far,
                              float trunc_dist, int subpix, kfx_stream stream);
int kfx_raycast_sdf_count_tracked_h(const kfx_volume* vol, kfx_sdf_summary* s, unsigned w, unsigned h, const float T_wc[12], const float K[4],
                                    float near, float far, float trunc_dist, int subpix, unsigned* d_bitmap, unsigned long long* d_counters,
                                    kfx_stream stream);
int kfx_raycast_sdf_levels_tracked_h(int n_levels, const kfx_image* const* depth, const kfx_image* const* norm, const kfx_image* const* img,
                                     const kfx_image* const* vbo, const kfx_volume* vol, kfx_sdf_summary* s, const float T_wc[12],
                                     const float* K, float near, float far, float trunc_dist, int subpix, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_SUMMARY_H_H */
