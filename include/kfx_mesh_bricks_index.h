/* kfx_mesh_bricks_index.h -- indexed output of the brick mesh (kfx_mesh_bricks.h): the marching-cubes vertices of packed 8 x 8 x 8
 * bricks welded on the device, so that the mesh of everything a moving volume has seen has one vertex per lattice edge and a face
 * list instead of three fresh vertices per triangle -- without a dense volume as large as the walk.  Same library (libkfx.so);
 * opt-in: kfx_mesh_bricks_plan / kfx_mesh_bricks_emit and their arrays stay as they are.
 *
 * Contract.  Let the BRICK SOUP be what kfx_mesh_bricks_emit writes for the same arguments: 3T vertices in its order -- cubes brick
 * by brick in ascending brick id, within a brick by ascending ci, within a cube the case table's triangle list.  Every soup vertex
 * lies on one LATTICE EDGE, kfx_mesh_index.h's, taken in frame cells: (componentwise minimum of the lattice coordinates of the two
 * corners its cube edge joins, axis in which they differ).  The indexed brick mesh is the sequential first-occurrence weld of the
 * brick soup, keyed by lattice edge: walk the soup in order; a key seen for the first time gets the next vertex id and takes that
 * soup vertex's position, normal and colour, bit for bit; faces[k] is the id of the key of soup vertex k.
 *   - verts[V][3], norms[V][3] and, with colour, colors[V][4] hold first-occurrence values.
 *   - faces[T][3] is uint32; triangles keep the brick soup's order and winding.
 *   - Keys are edges, not positions: two lattice edges whose vertices coincide in space (a corner value of exactly 0) stay two vertices.
 *   - V <= 3T < 2^32 by the plan's range check.
 * Absent bricks (unobserved: NaN, colour 0.5), the colour list, partial bricks, ids at or beyond the frame's brick count and half
 * cells: kfx_mesh_bricks.h's rules, unchanged -- this is the weld of that soup, whatever it is.
 *
 * AGAINST THE DENSE INDEXED MESH.  With D the dense volume of kfx_mesh_bricks.h's RESULT, kfx_mesh_emit_indexed (kfx_mesh_index.h)
 * on D gives the same set of welded vertices -- the same V, the same keys, the same T -- but NOT the same arrays: the soups differ in
 * order, so the ids differ, and so may the first occurrence.  Where the first cube around an edge in brick order is another than in
 * dense order, the vertex kept may differ in the last bit of a position (the cubes sharing an edge interpolate it from opposite
 * ends) and, next to unobserved cells, entirely in the normal (0 against a finite one).
 *
 * On the device: the OWNER of a lattice edge is the first cube in brick-soup order among the active cubes that contain it; vertex
 * ids run by owner cube in that order and, within a cube, by first use in its triangle list.  Brick order compares (brick id, ci): z
 * is most significant across bricks, x within one.  Where all four cubes around an edge are active the componentwise-minimum one is
 * first in both orders; where it is not active (it touches a NaN cell) the two diagonal cubes are ordered by the bricks they sit in,
 * so every active cube around the edge is looked up -- its brick through the home brick's 27-neighbour row of the plan's scratch,
 * then a binary search for its ci in that brick's segment of the compacted cube list -- and the first in list position taken.
 *
 * Three calls after kfx_mesh_bricks_plan (which gives totals = {active cubes, triangles} and fills `scratch`), with the same frame,
 * cell kind and lists:
 *   kfx_mesh_bricks_index_scratch_bytes(n, totals)   bytes of index scratch for a list of n bricks and these totals -- never a function
 *            of the frame.  With A = totals[0], xblk = ceil(A / 256) and round256 as in kfx_bricks.h:
 *                256 + round256(8 A) + 3 round256(4 A) + round256(4 n) + round256(8 xblk) + round256(16 xblk)
 *            -- a header; per active cube its ci, first triangle, case flag with the 12-bit mask of the edges it owns, and first
 *            vertex id (20 bytes); per listed brick the position of its first cube in the compacted list; the scan blocks' sums and
 *            offsets.  0 if the arguments are refused.
 *   kfx_mesh_bricks_index_plan      compacts the active cubes into the index scratch in brick order, records every brick's first cube
 *            position, finds every cube's owned edges and scans the counts; blocks until *n_verts = V is in host memory (one 16-byte
 *            read-back after the totals check's).  `scratch` needs the bytes of kfx_mesh_bricks_scratch_bytes(n, 0).
 *   kfx_mesh_bricks_emit_indexed    writes verts[V][3], norms[V][3], with colour colors[V][4] (kfx_mesh_bricks_emit's COLOUR: the
 *            colour brick list, `scratch` of kfx_mesh_bricks_scratch_bytes(n, n_color) bytes), and faces[T][3].
 * The lists must not change between the calls; `scratch` must be the plan's, unchanged, with its totals, and `index_scratch` the
 * index plan's, unchanged, with the same totals and its V: they are read back from the scratches and others refused with KFX_E_RANGE
 * before any launch.  Both scratches 256-byte aligned; the library never allocates.  No global atomics: ordering comes from the
 * stream, and the output is a function of the inputs.
 *
 * Unsorted or repeated ids on the device give an unspecified mesh but no access out of bounds, as the soup's: every list position
 * read from a scratch is range-checked before use and every output index compared with V or 3T before the store.
 *
 * Returns 0 or KFX_E_*, all before any HIP call: kfx_mesh_bricks_plan's refusals of the frame, the cell kind, the counts, the lists
 * and `scratch`; then null totals KFX_E_NULL; totals out of range (2^32/3 triangles or more, more cubes than triangles, more
 * vertices than 3T) KFX_E_RANGE; a null, short or misaligned index scratch KFX_E_NULL / KFX_E_SHAPE / KFX_E_ALIGN; a null n_verts
 * or -- with cubes to write -- output KFX_E_NULL, a misaligned output (4 bytes) KFX_E_ALIGN.  n == 0: totals must be (0, 0), V is 0,
 * nothing is launched; totals[0] == 0 likewise. */
#ifndef KFX_MESH_BRICKS_INDEX_H
#define KFX_MESH_BRICKS_INDEX_H

#include "kfx_mesh_bricks.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t kfx_mesh_bricks_index_scratch_bytes(unsigned long long n, const unsigned long long totals[2]);
int kfx_mesh_bricks_index_plan(const kfx_volume* frame, int cell, const unsigned* ids, const void* cells, unsigned long long n,
                               const void* scratch, size_t scratch_bytes, const unsigned long long totals[2], void* index_scratch,
                               size_t index_scratch_bytes, unsigned long long* n_verts, kfx_stream stream);
int kfx_mesh_bricks_emit_indexed(const kfx_volume* frame, int cell, const unsigned* ids, const void* cells, unsigned long long n,
                                 const unsigned* color_ids, const void* color_cells, unsigned long long n_color, void* scratch,
                                 size_t scratch_bytes, const void* index_scratch, size_t index_scratch_bytes,
                                 const unsigned long long totals[2], unsigned long long n_verts, float* verts, float* norms, float* colors,
                                 unsigned* faces, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_MESH_BRICKS_INDEX_H */
