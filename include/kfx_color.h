/* kfx_color.h -- colour mode at the speed of the grey path: the colour SdfFuse that keeps the brick summary of include/kfx.h
 * (kfx_sdf_summary) current, and the colour image of any rendering as a pass over its depth image.  Same library (libkfx.so);
 * kfx_sdf_fuse_color, kfx_raycast_sdf_color and kfx_color_reset, the reference's three colour operators, are declared in kfx.h. */
#ifndef KFX_COLOR_H
#define KFX_COLOR_H

#include "kfx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kfx_sdf_fuse_color with the brick summary kept current: SDF and colour cells bit-identical to kfx_sdf_fuse_color with the
 * same arguments, in both numerics modes.  The contract is kfx_sdf_fuse_tracked's: views of the summary's volume may be passed;
 * a view that does not start on multiples of 8 cells, or a launch that takes the untiled kernel, invalidates the summary
 * itself; a summary created for half cells is rejected with KFX_E_SHAPE and a null one with KFX_E_NULL before anything is
 * launched. */
int kfx_sdf_fuse_color_tracked(const kfx_volume* vol, const kfx_volume* colorvol, kfx_sdf_summary* s, const kfx_image* depth,
                               const kfx_image* norm, const float T_cw[12], const float K[4], const kfx_image* img, const float T_iw[12],
                               const float Kimg[4], float trunc_dist, float max_w, float mincostheta, unsigned flags, kfx_stream stream);

/* The colour image of renderings that were already marched.  For level l and every pixel (u, v) with depth[l](u, v) > 0,
 * img[l](u, v) = colorvol.GetUnitsTrilinearClamped(c_w + ray_w * depth): the value kfx_raycast_sdf_color writes there (bit for
 * bit in exact numerics).  Other pixels are left alone: the march wrote the 0 of "no hit", the colour variant's value too.  So
 * kfx_raycast_sdf[_tracked] or kfx_raycast_sdf_levels[_tracked] followed by this call renders colour.  depth[l] and img[l] are
 * float images of equal size; K holds 4 floats per level; colorvol has its own box, as in kfx_raycast_sdf_color;
 * 1 <= n_levels <= 8.  One launch for all levels. */
int kfx_raycast_color_hits(int n_levels, const kfx_image* const* depth, const kfx_image* const* img, const kfx_volume* colorvol,
                           const float T_wc[12], const float* K /* 4 per level */, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_COLOR_H */
