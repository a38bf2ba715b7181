/* kfx_slab_color.h -- colour mode on Z-slabs: the reference application's fuse_color mode (colour SdfFuse, colour RaycastSdf) on the
 * partition of kfx_slab.h, bit-identical to kfx_sdf_fuse_color / kfx_raycast_sdf_color on the whole volume in both numerics modes.
 * Same library (libkfx.so); fp32 SDF cells only.
 *
 * The colour volume (BoundedVolume<float>) is partitioned exactly like the SDF volume: rank r stores the colour planes [s0, s1) of the
 * layout as a volume of its own, with the local box.  The FULL colour volume has the SDF volume's dimensions and box -- so a rank's
 * colour slab has its SDF slab's w, h, d and box; anything else is KFX_E_SHAPE before any launch.  (The single-volume operators allow a
 * colour volume with a box of its own; here equal geometry is what makes the two planes of a hit's colour sample a subset of the three
 * planes of its gradient stencil, which the rank that finalises the hit holds anyway.)
 *
 * Every entry point checks its arguments before any HIP call. */
#ifndef KFX_SLAB_COLOR_H
#define KFX_SLAB_COLOR_H

#include "kfx_slab.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kfx_sdf_fuse_color on planes [slab->z_offset, slab->z_offset + vol->d) of the volume `slab` describes: voxel positions by the full
 * volume's expression, so stored plane k of `vol` and of `colorvol` gets the bits of plane z_offset + k of the monolithic colour
 * fuse.  Extents: the reference's colour launch on the whole volume -- x, y truncated to multiples of 16, every plane
 * (KFX_FUSE_FULL_EXTENT lifts the truncation; KFX_FUSE_SLAB_EXTENT is accepted and means the same as 0 here: the colour launch has no
 * truncation in z). */
int kfx_sdf_fuse_color_slab(const kfx_volume* vol, const kfx_volume* colorvol, const kfx_slab* slab, const kfx_image* depth,
                            const kfx_image* norm, const float T_cw[12], const float K[4], const kfx_image* img, const float T_iw[12],
                            const float Kimg[4], float trunc_dist, float max_w, float mincostheta, unsigned flags, kfx_stream stream);

/* kfx_raycast_sdf_slab / kfx_raycast_sdf_slab_tiles (kfx.h) whose finalising rank writes the colour volume's trilinear sample at the
 * hit -- the value kfx_raycast_sdf_color writes to img -- into the shade plane instead of the Phong shade.  The colour travels where
 * the shade travels: the result plane, kfx_raycast_state_to_images, the strips of the final exchange. */
int kfx_raycast_sdf_slab_color(float* state, int init, const kfx_volume* vol, const kfx_volume* colorvol, const kfx_slab* slab, int own_lo,
                               int own_hi, int w, int h, const float T_wc[12], const float K[4], float near, float far, float trunc_dist,
                               int subpix, kfx_stream stream);
int kfx_raycast_sdf_slab_tiles_color(float* state, float* result, size_t plane_stride, int rows_per_tile, int v0, int v1, int init, int* fin,
                                     int claim_misses, const float* adopt_lo, const float* adopt_hi, int layout_flags, const kfx_volume* vol,
                                     const kfx_volume* colorvol, const kfx_slab* slab, int own_lo, int own_hi, int w, int h,
                                     const float T_wc[12], const float K[4], float near, float far, float trunc_dist, int subpix,
                                     kfx_stream stream);

/* kfx_slab_raycast_exact_tiled (kfx_slab.h) with this rank's colour slab: every rank returns with the three images of
 * kfx_raycast_sdf_color on the whole volumes, bit for bit.  Same scratch, same messages, same collectives as the grey hand-over. */
int kfx_slab_raycast_exact_tiled_color(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, void* scratch,
                                       const kfx_volume* local, const kfx_volume* color_local, const kfx_slab_layout* L, const float T_wc[12],
                                       const float K[4], float near, float far, float trunc_dist, int subpix, int tiles, kfx_comm* comm,
                                       kfx_stream stream, int* h_open, int* steps_out);

/* Colour mode of a slab rank's frame object.  Call once after kfx_slab_frame_create (and between frames to change the views):
 * color_local = this rank's colour slab (planes [layout.s0, layout.s1), the geometry of the frame's SDF slab), rgb = the frame's RGB
 * image (uchar3 pixels, device memory; its contents may change between steps), Kimg = the colour camera's intrinsics, T_cd = colour
 * camera <- depth camera (12 floats; null: identity).  From then on kfx_slab_frame_step integrates with the colour SdfFuse at
 * T_iw = T_cd * T_cw and renders colour: the colour hand-over (raycast EXACT), or kfx_raycast_sdf_color per slab whose merge carries
 * img as it does the shade (COMPOSITE).  With halo EXCHANGE the colour volume's ghost planes are fetched after the SDF volume's, in
 * that order on every rank.  kfx_slab_frame_reset also resets the colour slab (0.5).  color_local = NULL returns the frame to grey
 * (the other arguments are ignored).  Every rank of the frame's communicator makes the same call. */
int kfx_slab_frame_set_color(kfx_slab_frame* f, const kfx_volume* color_local, const kfx_image* rgb, const float Kimg[4], const float* T_cd /* null: identity */);

#ifdef __cplusplus
}
#endif
#endif /* KFX_SLAB_COLOR_H */
