/* kfx_raycast_bricks.h -- RaycastSdf straight from packed 8 x 8 x 8 bricks: the rendering of everything a moving volume has seen (the
 * bricks it spilled, kfx_bricks.h, together with those of its live box) from any pose, without a dense volume as large as the walk.
 * Same library (libkfx.so); kept out of kfx.h.
 *
 * FRAME.  kfx_mesh_bricks.h's: a virtual dense volume, dimensions (w, h, d) and a box, passed as a kfx_volume of which ptr, pitch and
 * img_pitch are ignored (null / zero will do).  Its brick grid is kfx_bricks.h's: nbx = ceil(w / 8) ..., id = (bz * nby + by) * nbx + bx,
 * partial last bricks where a dimension is no multiple of 8.  Dimensions as kfx_raycast_sdf accepts them (3 .. 65535), 2^31 - 1 bricks
 * at the most.
 *
 * INPUT.  n bricks as kfx_bricks_pack writes them for a view of these dimensions: ids[n] uint32, ascending; cells[n][8][8][8], x
 * fastest, in the cell's bytes (KFX_CELL_F32 or KFX_CELL_F16).  Optionally a second list (color_ids, color_cells, n_color) of
 * KFX_CELL_COLOR bricks (2048 bytes each) on the same frame.  ABSENT MEANS UNOBSERVED: a cell of the frame in no listed brick has the
 * value NaN (colour: 0.5).  Cells of a partial brick's payload outside (w, h, d) are never read.  An id at or beyond the frame's brick
 * count is skipped; unsorted or repeated ids give unspecified images (no access out of bounds either way: every probe of a table
 * stays inside it, and a position it yields is used only if it is below n).
 *
 * RESULT.  Let D be a dense volume of the frame's dimensions and box, kfx_sdf_reset(D, NaN) (half cells: kfx_sdf_reset_h), then
 * kfx_bricks_unpack(D, ids, cells, n).  kfx_raycast_bricks writes exactly what kfx_raycast_sdf (kfx_raycast_sdf_h) writes for D with the
 * same images, pose, intrinsics, near, far, trunc_dist and subpix: the same bits in every pixel of depth, normal and shade, the no-hit
 * values included, and nothing outside the images' w x h.  So a sample with an absent cell among its eight is NaN, steps by trunc_dist
 * and cannot end in a hit, and a hit whose gradient stencil reaches an absent brick has the normal of a vanishing gradient, (0, 0, 1)
 * in the world.  The plain march has one numerics mode: this holds under either kfx_set_math_mode.
 * color != 0: what kfx_raycast_sdf_color writes for D and a colour volume C of the frame's dimensions and box, filled with 0.5, then
 * the colour bricks unpacked -- img is C's trilinear sample at the hit.  n_color == 0: the img of every hit is 0.5.
 *
 * Two calls.  kfx_raycast_bricks_plan builds, on the device, what a ray needs to find a brick from a cell coordinate: an
 * open-addressing hash table from brick id to list position (linear probing; filled by one kernel with a 32-bit compare-and-swap on the
 * id word; ids that are no brick of the frame are not inserted), and a second one for the colour list when n_color > 0.  No read-back:
 * the call returns when the work is enqueued.  kfx_raycast_bricks, given the same lists and the plan's scratch, marches one ray per
 * pixel; it reads the scratch and never writes it, so one plan serves any number of views, poses and image sizes.
 *
 *   scratch  device memory of the caller, 256-byte aligned, of kfx_raycast_bricks_scratch_bytes(n, n_color) bytes -- a function of the
 *            brick counts alone, never of the frame.  With cap(0) = 0, cap(m) = the smallest power of two >= 2 m, and round256 as in
 *            kfx_bricks.h:
 *                256 + round256(8 cap(n)) + round256(8 cap(n_color))
 *            -- a header and 8 bytes {id, position} per table entry: 16 to 32 bytes per 4096-byte fp32 brick.  The header block holds,
 *            as written by the plan's kernel, {n, n_color} (two uint32) and {cap(n), cap(n_color)} (two uint64 at byte 8).  It is a
 *            record, not a key: reading it would be a read-back per view, so kfx_raycast_bricks recomputes the layout from its own n
 *            and n_color and compares SIZES only (a scratch below the bytes of its arguments is refused); a scratch planned for other
 *            lists of the same counts gives unspecified images, inside the bounds stated above.
 *            The library never allocates, and no call touches memory in proportion to the frame.
 *   ids, color_ids 4-byte aligned; cells, color_cells 16-byte aligned; images as kfx_raycast_sdf's.
 *
 * Returns 0 or KFX_E_*, all refusals before any HIP call, in this order: a null T_wc or K KFX_E_NULL; the images as kfx_raycast_sdf
 * checks them (null KFX_E_NULL; smaller than img, a pitch below a row, above 2^30 KFX_E_SHAPE; misaligned KFX_E_ALIGN); a null frame
 * KFX_E_NULL; an unknown cell kind KFX_E_RANGE; frame dimensions below 3 or above 65535 KFX_E_SHAPE; more than 2^31 - 1 bricks in
 * the frame KFX_E_RANGE; color != 0 with half cells KFX_E_RANGE (kfx_raycast_sdf_color takes fp32 cells); more than 2^31 - 1 entries
 * in a list KFX_E_RANGE; with entries, a null list KFX_E_NULL, a misaligned one KFX_E_ALIGN; a null scratch KFX_E_NULL, too little of
 * it KFX_E_SHAPE, a misaligned one KFX_E_ALIGN.  (The plan: the same without pose, images, cell kind and payloads.)
 * n == 0: every pixel is a miss; the kernel is launched, the lists are never read.  An image with w == 0 or h == 0 launches nothing. */
#ifndef KFX_RAYCAST_BRICKS_H
#define KFX_RAYCAST_BRICKS_H

#include "kfx_bricks.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of scratch for lists of n SDF bricks and n_color colour bricks; 0 if the counts are refused */
size_t kfx_raycast_bricks_scratch_bytes(unsigned long long n, unsigned long long n_color);
/* the tables from brick id to list position, on the device; no read-back */
int kfx_raycast_bricks_plan(const kfx_volume* frame, const unsigned* ids, unsigned long long n, const unsigned* color_ids,
                            unsigned long long n_color, void* scratch, size_t scratch_bytes, kfx_stream stream);
/* kfx_raycast_sdf / _h / _color of the volume the bricks would unpack into; cell: KFX_CELL_F32 or KFX_CELL_F16, the kind of `cells` */
int kfx_raycast_bricks(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const kfx_volume* frame, int cell,
                       const unsigned* ids, const void* cells, unsigned long long n, const unsigned* color_ids, const void* color_cells,
                       unsigned long long n_color, int color, const void* scratch, size_t scratch_bytes, const float T_wc[12],
                       const float K[4], float near, float far, float trunc_dist, int subpix, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_RAYCAST_BRICKS_H */
