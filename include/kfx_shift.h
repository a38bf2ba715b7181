/* kfx_shift.h -- moving volume: shift the cells of a BoundedVolume by whole voxels, in place, on the device, so that the box can
 * follow the camera without a round trip of the volume through the host.  Same library (libkfx.so); kept out of kfx.h.
 *
 * For shift = (sx, sy, sz) in whole cells, on a volume or any view of one (SubVolume, Z-slab view):
 *     new(x, y, z) = old(x + sx, y + sy, z + sz)   where that source lies inside the view,
 *     new(x, y, z) = the fill value                 elsewhere.
 * Retained cells are copied byte for byte (NaN payloads included).  Bytes outside the view's cells -- pitch padding, the neighbours
 * of a sub-view -- are never written.  shift == 0 launches nothing; |s| >= the extent in any axis is one fill.
 *
 *   cell     KFX_CELL_F32 (roo::SDF_t, 8 bytes; fill = {fill, 0}, the bytes kfx_sdf_reset(vol, fill) writes), KFX_CELL_F16
 *            (roo::SDF_h, 4 bytes; the bytes of kfx_sdf_reset_h(vol, fill)) or KFX_CELL_COLOR (BoundedVolume<float>, 4 bytes; fill
 *            itself).  The application passes NaN for SDF cells and 0.5 for colour.
 *   scratch  device memory supplied by the caller, 256-byte aligned; the library never allocates.  Needed only where
 *            kfx_volume_shift_scratch_bytes() is not 0 (sz == 0): then at least that many bytes -- one packed z-plane, w * h * cell
 *            bytes rounded up to 256.  A larger scratch is used for larger chunks (fewer launches).
 *
 * The plan (why in place is safe).  Workgroups of one launch run in no order, so no launch reads cells that it writes; launches on
 * one stream are ordered.  The planes that have a source are visited in chunks of P whole z-planes, ascending z when sz >= 0,
 * descending when sz < 0, and each chunk is
 *     DIRECT   (sz != 0, P = |sz|): one launch that reads planes [z0 + sz, z1 + sz) of the volume and writes planes [z0, z1), shifted
 *              in x and y, filling the cells whose source is outside.  |sz| >= P makes the two plane ranges disjoint.  No scratch;
 *              one read and one write per cell.
 *     STAGE + PLACE (sz == 0, P = the planes the scratch holds): STAGE copies planes [z0, z1) packed into the scratch; PLACE reads the
 *              scratch and writes planes [z0, z1) shifted in x and y, and fills.  Each reads one buffer and writes the other.
 * Destination chunk k overwrites only planes that are sources of chunks up to and including k: with sz > 0 and ascending z the
 * sources of chunk k are planes >= z0 + sz > z0, so every plane below z1 is the source of chunk k or an earlier one -- already read
 * (or, staged, sitting in the scratch); descending z mirrors it.  Planes whose sources all lie outside the view are one FILL, issued
 * LAST: they are the sources of the last chunks.
 *
 * The box: kfx_volume_shift_box gives boxmin' = VoxelPositionInUnits(sx, sy, sz), boxmax' = VoxelPositionInUnits(w - 1 + sx,
 * h - 1 + sy, d - 1 + sz), each coordinate by the reference's fp32 expression min + size * i / (float)(dim - 1).  Retained voxels keep
 * their data, while their nominal position may move by an ulp of the coordinate per shift; on lattices whose positions are exact in
 * fp32 it does not move at all.  kfx_volume_shift does NOT change vol->boxmin / boxmax (the volume argument is const): the caller
 * stores the new box.
 *
 * A brick summary (kfx_sdf_summary) is keyed by the volume's storage and holds no box: a caller with its own summary calls
 * kfx_volume_shift and then kfx_sdf_summary_rebuild.  kfx_frame_shift does both for a kfx_frame.
 *
 * Returns 0 or KFX_E_*, all before any HIP call: a null volume, shift, or -- where scratch is needed -- null scratch KFX_E_NULL; an
 * unknown cell kind KFX_E_RANGE; the volume's own rules (KFX_E_SHAPE / KFX_E_ALIGN); a scratch below the minimum KFX_E_SHAPE; a
 * misaligned scratch KFX_E_ALIGN. */
#ifndef KFX_SHIFT_H
#define KFX_SHIFT_H

#include "kfx_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KFX_CELL_COLOR 2   /* float: BoundedVolume<float>, the colour volume */

#define KFX_SHIFT_FILL   0   /* dst planes [dst_z0, dst_z1) of the volume = fill */
#define KFX_SHIFT_DIRECT 1   /* volume planes [src_z0, src_z1) -> volume planes [dst_z0, dst_z1), shifted in x and y */
#define KFX_SHIFT_STAGE  2   /* volume planes [src_z0, src_z1) -> scratch planes [dst_z0, dst_z1), packed, unshifted */
#define KFX_SHIFT_PLACE  3   /* scratch planes [src_z0, src_z1) -> volume planes [dst_z0, dst_z1), shifted in x and y */

typedef struct kfx_shift_step {
    int kind;             /* KFX_SHIFT_* */
    int dst_z0, dst_z1;   /* planes written: of the volume, or (STAGE) of the scratch */
    int src_z0, src_z1;   /* planes read: of the volume, or (PLACE) of the scratch; FILL: 0, 0 */
} kfx_shift_step;

/* the minimum scratch of these arguments; 0 where none is needed or the arguments are refused */
size_t kfx_volume_shift_scratch_bytes(const kfx_volume* vol, int cell, const int shift[3]);
/* host only: the box of the shifted volume */
int kfx_volume_shift_box(const kfx_volume* vol, const int shift[3], float boxmin_out[3], float boxmax_out[3]);
/* host only: the launches kfx_volume_shift enqueues for these arguments, in order.  *n_steps_out = their number; the first
 * min(that, max_steps) are written to steps_out (which may be null with max_steps 0).  A volume of d planes takes at most 2 d + 1. */
int kfx_volume_shift_plan(const kfx_volume* vol, int cell, const int shift[3], size_t scratch_bytes, kfx_shift_step* steps_out, int max_steps,
                          int* n_steps_out);
int kfx_volume_shift(const kfx_volume* vol, int cell, const int shift[3], float fill, void* scratch, size_t scratch_bytes, kfx_stream stream);
/* shifts cfg.vol of the frame (fill NaN), stores the new box in the frame and, when the frame tracks, rebuilds its summary */
int kfx_frame_shift(kfx_frame* frame, const int shift[3], void* scratch, size_t scratch_bytes, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_SHIFT_H */
