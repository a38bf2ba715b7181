/* kfx_mesh.h -- mesh extraction as SaveMesh and ExtractMesh call it: roo::SaveMesh's marching cubes (reference
 * include/kangaroo/MarchingCubes.h) for fp32 and half-cell volumes, whole or as one Z-slab of a partitioned volume, counted, scanned
 * and compacted on the device.  Same library (libkfx.so) as kfx.h, whose kfx_mc_count / kfx_mc_emit (a byte per cube, compacted by
 * the caller; fp32, whole volumes) stay beside it as the tests' independent comparator.
 *
 * Two calls.  kfx_mesh_plan counts the active cubes and triangles per SEGMENT (up to 64 consecutive cubes along z in one (x, y)
 * column) and scans the counts in the reference's emission order ((x*(h-1) + y)*(d-1) + z); it blocks until the totals are in host
 * memory (one 16-byte read-back).  The caller sizes its buffers from them and kfx_mesh_emit writes, in emission order:
 *   cube_index[totals[0]]   int64: the global index of every cube with triangles
 *   tri_offset[totals[0]]   uint32: its first triangle
 *   verts[3 totals[1]][3], norms[3 totals[1]][3] and, with a colour volume, colors[3 totals[1]][4]: three vertices per triangle.
 * The volume must not change between the two calls, and the scratch of a plan must be passed unchanged to its emit, with the
 * plan's totals: kfx_mesh_emit reads them back from the scratch (16 bytes) and refuses others with KFX_E_RANGE.
 *
 *   cell     KFX_CELL_F32 (roo::SDF_t) or KFX_CELL_F16 (roo::SDF_h).  Half cells: the mesh of the WIDENED volume, every half
 *            converted exactly to float (what the reference's SaveMesh<T> does through operator float).
 *   slab     NULL: every cube of `vol`.  The arrays are those of kfx_mc_count -> prefix sum -> kfx_mc_emit, bit for bit.
 *            Otherwise `vol` holds planes [slab->z_offset, slab->z_offset + vol->d) of the volume `slab` describes (x / y extents
 *            and box those of `vol`, as for kfx_sdf_fuse_slab); the call meshes the cubes whose lower plane lies in
 *            [own_lo, min(own_hi, full_d - 1)).  Positions and normals use the full volume's expressions, so each triangle is
 *            bit-identical to the same cube's triangle in the single-volume mesh, and cube_index is the global index.  The stored
 *            planes must cover [own_lo - 2, own_hi + 2) within [0, full_d) -- the corners' planes z, z + 1 and the normals' gradient
 *            stencil (base plane clamp(floor(vertex z), 1, full_d - 2) and one plane either side) -- so a ghost of 2 planes per
 *            side suffices (a vertex's colour reads planes up to z + 2, inside the stencil's); otherwise KFX_E_RANGE before any launch.
 *   colorvol a BoundedVolume<float>; sampled only when it IsValid() (every dimension >= 8) and `colors` is not null.  With a slab
 *            (fp32 cells): the rank's colour slab -- the same planes of a colour volume with the SDF volume's dimensions and box, so
 *            it has the w, h, d and box of `vol` (KFX_E_SHAPE otherwise); colours equal the single volume's bit for bit.
 *   scratch  device memory of kfx_mesh_scratch_bytes() bytes, 256-byte aligned: the per-segment counts (2 bytes each) and the
 *            scan's block sums and offsets.  The library never allocates.  2048^3 cells, whole volume: 274 460 416 bytes (512^3: 4 277 504).
 *
 * Returns 0 or KFX_E_*: null pointers KFX_E_NULL, an unknown cell kind KFX_E_RANGE, too little scratch KFX_E_SHAPE, all before any
 * HIP call; a mesh of 2^32/3 triangles or more (32-bit vertex offsets) KFX_E_RANGE from kfx_mesh_plan, with the totals filled in.
 *
 * Indexed output (one vertex per lattice edge and a face list, welded on the device from the same plan): kfx_mesh_index.h. */
#ifndef KFX_MESH_H
#define KFX_MESH_H

#include "kfx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KFX_CELL_F32 0   /* SDF_t {float val; float w;} */
#define KFX_CELL_F16 1   /* SDF_h {half val; half w;}   */

/* bytes of scratch a plan of these arguments needs; 0 if the arguments are refused */
size_t kfx_mesh_scratch_bytes(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi);
/* count + scan; totals[0] = active cubes, totals[1] = triangles */
int kfx_mesh_plan(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi,
                  void* scratch, size_t scratch_bytes, unsigned long long totals[2], kfx_stream stream);
/* compact + emit into caller buffers sized from the plan's totals (passed back here: nothing is written beyond them) */
int kfx_mesh_emit(const kfx_volume* vol, int cell, const kfx_slab* slab, int own_lo, int own_hi, const kfx_volume* colorvol,
                  const void* scratch, size_t scratch_bytes, const unsigned long long totals[2], long long* cube_index,
                  unsigned* tri_offset, float* verts, float* norms, float* colors, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_MESH_H */
