/* kfx_mesh_index.h -- indexed output of the planned mesh extraction (kfx_mesh.h): marching-cubes vertices welded on the device, so
 * that a mesh has one vertex per lattice edge and a face list instead of three fresh vertices per triangle.  Same library
 * (libkfx.so); opt-in: kfx_mesh_plan / kfx_mesh_emit and their arrays stay as they are.
 *
 * Contract.  Let the SOUP be what kfx_mesh_emit writes for the same arguments: 3T vertices in emission order.  Every soup vertex
 * lies on one LATTICE EDGE: the cube is (x, y, z), the case-table edge e joins corners c0 and c1, and the lattice edge is
 * (componentwise minimum of the two corners' lattice coordinates, axis in which they differ).  The indexed mesh is the sequential
 * first-occurrence weld of the soup, keyed by lattice edge: walk the soup in order; a key seen for the first time gets the next
 * vertex id and takes that soup vertex's position, normal and colour, bit for bit; faces[k] is the id of the key of soup vertex k.
 *   - verts[V][3], norms[V][3], colors[V][4] hold first-occurrence values.  Later copies of an edge are dropped: the cubes sharing
 *     an edge interpolate it from opposite ends, so a copy may differ in the last bit of a position, and next to unobserved cells
 *     entirely in the normal (0 against a finite one) -- which is why "first" is part of the contract.
 *   - faces[T][3] is uint32; triangles keep the soup's order and winding.
 *   - Keys are edges, not positions: two lattice edges whose vertices coincide in space (a corner value of exactly 0) stay two vertices.
 *   - A slab call welds within the cubes it meshes: a rank's indexed mesh is the weld of that rank's soup, and a vertex on a slab
 *     boundary exists once per rank that uses it.
 *   - V <= 3T < 2^32 by the plan's range check.
 * On the device: the OWNER of a lattice edge is the first cube in emission order ((x*(h-1) + y)*(d-1) + z) among the meshed cubes
 * that contain it; vertex ids run by owner cube in emission order and, within a cube, by first use in its triangle list.
 *
 * Three calls after kfx_mesh_plan (which gives totals = {active cubes, triangles} and fills `scratch`):
 *   kfx_mesh_index_scratch_bytes  bytes of index scratch for these totals: 20 per active cube (its index, first triangle, case flag
 *                                 with the 12-bit mask of the edges it owns, first vertex id) plus 24 per 256 active cubes (scan
 *                                 partials) plus 256.  Nothing per voxel or per lattice edge.  0 if the arguments are refused.
 *   kfx_mesh_index_plan           compacts the active cubes into the index scratch, finds every cube's owned edges (binary searches
 *                                 in the ascending cube list for the up to three cubes that precede it around an edge), scans the
 *                                 counts; blocks until *n_verts = V is in host memory (one 16-byte read-back after the totals check's).
 *   kfx_mesh_emit_indexed         writes verts[V][3], norms[V][3], with a colour volume colors[V][4], and faces[T][3].
 * The volume must not change between the calls; `scratch` must be the plan's, unchanged, with its totals, and `index_scratch` the
 * index plan's, unchanged, with the same totals and its V: both are read back from the scratch and others refused with KFX_E_RANGE.
 * vol, cell, slab, own_lo, own_hi, colorvol: as in kfx_mesh.h.  Both scratches 256-byte aligned; the library never allocates.
 *
 * Returns 0 or KFX_E_*: null pointers KFX_E_NULL, an unknown cell kind or totals out of range (2^32/3 triangles or more, more cubes
 * than triangles, more vertices than 3T) KFX_E_RANGE, too little scratch KFX_E_SHAPE, all before any HIP call. */
#ifndef KFX_MESH_INDEX_H
#define KFX_MESH_INDEX_H

#include "kfx_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t kfx_mesh_index_scratch_bytes(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi,
                                    const unsigned long long totals[2]);
int kfx_mesh_index_plan(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi, const void* scratch,
                        size_t scratch_bytes, const unsigned long long totals[2], void* index_scratch, size_t index_scratch_bytes,
                        unsigned long long* n_verts, kfx_stream stream);
int kfx_mesh_emit_indexed(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi, const kfx_volume* colorvol,
                          const void* index_scratch, size_t index_scratch_bytes, const unsigned long long totals[2],
                          unsigned long long n_verts, float* verts, float* norms, float* colors, unsigned* faces, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_MESH_INDEX_H */
