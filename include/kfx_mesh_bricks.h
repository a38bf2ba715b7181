/* kfx_mesh_bricks.h -- marching cubes straight from packed 8 x 8 x 8 bricks: the mesh of everything a moving volume has seen (the
 * bricks it spilled, kfx_bricks.h, together with those of its live box) without a dense volume as large as the walk.  Same library
 * (libkfx.so); kept out of kfx.h and kfx_mesh.h.
 *
 * FRAME.  A virtual dense volume: dimensions (w, h, d) and a box, passed as a kfx_volume of which ptr, pitch and img_pitch are ignored
 * (null / zero will do).  Its brick grid is kfx_bricks.h's: nbx = ceil(w / 8) ..., id = (bz * nby + by) * nbx + bx, partial last bricks
 * where a dimension is no multiple of 8.  Dimensions as kfx_mesh_plan accepts them (3 .. 65535), 2^31 - 1 bricks at the most.
 *
 * INPUT.  n bricks as kfx_bricks_pack writes them for a view of these dimensions: ids[n] uint32, strictly ascending;
 * cells[n][8][8][8], x fastest, in the cell's bytes (KFX_CELL_F32 or KFX_CELL_F16).  ABSENT MEANS UNOBSERVED: a cell of the frame in
 * no listed brick has the value NaN -- what kfx_sdf_reset(vol, NaN) and a shift write.  Cells of a partial brick's payload outside
 * (w, h, d) are never read.  An id at or beyond the frame's brick count is skipped; unsorted or repeated ids give an unspecified
 * mesh (no access out of bounds either way: a cube's triangles go into the slots the plan counted for it, and no further).
 *
 * RESULT.  Let D be a dense volume of the frame's dimensions and box, kfx_sdf_reset(D, NaN), then kfx_bricks_unpack(D, ids, cells, n).
 * The brick mesh is the soup kfx_mesh_plan / kfx_mesh_emit (kfx_mesh.h, slab = NULL) produce on D: the same active cubes and for each
 * the same triangles, vertices, normals and colours, bit for bit (half cells: the exactly widened volume's).  So a cube that touches
 * an absent brick has no triangles, and a normal whose gradient stencil reaches into one is (0, 0, 0).  Only the ORDER differs: cubes
 * are listed brick by brick in ascending brick id -- a cube belongs to the brick that holds its minimum-corner cell -- and within a
 * brick by ascending dense index ci = (x * (h - 1) + y) * (d - 1) + z, x, y, z in frame cells.  The outputs are kfx_mesh_emit's:
 *   cube_index[totals[0]]   int64: that dense ci
 *   tri_offset[totals[0]]   uint32: the cube's first triangle
 *   verts[3 totals[1]][3], norms[3 totals[1]][3] and, with colour, colors[3 totals[1]][4]: three vertices per triangle.
 *
 * COLOUR.  Written when `colors` is not null and the frame IsValid() (every dimension >= 8): a second brick list (color_ids,
 * color_cells, n_color) of KFX_CELL_COLOR bricks (2048 bytes each) on the same frame.  An absent colour brick reads as 0.5, what
 * kfx_color_reset writes: the colours are those of kfx_mesh_emit with a colour volume C of the frame's dimensions and box, filled
 * with 0.5, then unpacked.  n_color == 0: every colour is 0.5.  Both SDF cell kinds.
 *
 * Two calls, as kfx_mesh.h.  kfx_mesh_bricks_plan finds every listed brick's 26 neighbours in the list (binary searches), counts
 * each brick's active cubes and triangles, scans them in the order above and blocks until the totals are in host memory (one
 * 16-byte read-back).  The caller sizes its buffers; kfx_mesh_bricks_emit, given the same lists, the plan's scratch unchanged and the
 * plan's totals (read back from the scratch, 16 bytes; others are refused with KFX_E_RANGE before any launch), writes them.
 *
 *   scratch  device memory of the caller, 256-byte aligned, of kfx_mesh_bricks_scratch_bytes(n, n_color) bytes -- a function of the
 *            brick counts alone, never of the frame.  With nblk = ceil(n / 256) and round256 as in kfx_bricks.h:
 *                256 + round256(108 n) + round256(4 n) + round256(8 nblk) + round256(16 nblk) + (n_color ? round256(108 n) : 0)
 *            -- a header, 27 list positions per brick (itself and its neighbours), a count per brick, the scan blocks' sums and
 *            offsets, and with a colour list the 27 positions in that list.  About 112 bytes per 4096-byte fp32 brick (220 with colour).
 *            A plan needs the bytes of n_color = 0 only.  The library never allocates, and no call touches memory in proportion to
 *            the frame: scratch and outputs are bounded by this function of n, n_color and 16 bytes per active cube + 72 (colour: 120)
 *            per triangle.
 *   ids, color_ids 4-byte aligned; cells, color_cells 16-byte aligned.
 *
 * Returns 0 or KFX_E_*, all before any HIP call: a null frame, scratch, totals or -- with entries -- list KFX_E_NULL; an unknown
 * cell kind, more than 2^31 - 1 bricks in the frame or entries in a list KFX_E_RANGE; frame dimensions kfx_mesh_plan would refuse or
 * too little scratch KFX_E_SHAPE; a misaligned scratch, list or output KFX_E_ALIGN.  n == 0: totals (0, 0), nothing is launched.  A
 * mesh of 2^32/3 triangles or more: KFX_E_RANGE from the plan, with the totals filled in. */
#ifndef KFX_MESH_BRICKS_H
#define KFX_MESH_BRICKS_H

#include "kfx_bricks.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of scratch for lists of n SDF bricks and n_color colour bricks; 0 if the counts are refused */
size_t kfx_mesh_bricks_scratch_bytes(unsigned long long n, unsigned long long n_color);
/* neighbour table + count + scan; totals[0] = active cubes, totals[1] = triangles */
int kfx_mesh_bricks_plan(const kfx_volume* frame, int cell, const unsigned* ids, const void* cells, unsigned long long n, void* scratch,
                         size_t scratch_bytes, unsigned long long totals[2], kfx_stream stream);
/* compact + emit into caller buffers sized from the plan's totals (passed back here: nothing is written beyond them) */
int kfx_mesh_bricks_emit(const kfx_volume* frame, int cell, const unsigned* ids, const void* cells, unsigned long long n,
                         const unsigned* color_ids, const void* color_cells, unsigned long long n_color, void* scratch,
                         size_t scratch_bytes, const unsigned long long totals[2], long long* cube_index, unsigned* tri_offset,
                         float* verts, float* norms, float* colors, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_MESH_BRICKS_H */
