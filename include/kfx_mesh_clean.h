/* kfx_mesh_clean.h -- clean-up of an indexed mesh in device memory: its connected components, and the removal of the small ones with the
 * rest compacted.  Same library (libkfx.so); the extraction calls (kfx_mesh_index.h, kfx_mesh_bricks_index.h) stay as they are.
 *
 * Input.  An indexed mesh as either *_emit_indexed writes it: V vertices and faces[T][3] of uint32 ids, V <= 3T < 2^32; any face list
 * with ids < V is accepted, it need not come from this library.  norms[V][3] and colors[V][4] are optional.
 *
 * Components.  Two vertices are connected when a face contains both; a component is a class of the transitive closure.  Ids decide,
 * not positions: two lattice edges whose vertices coincide in space are two vertices (kfx_mesh_index.h) and may fall into two
 * components.  A vertex in no face is a component of its own with 0 faces; a degenerate face (a repeated id) counts as a face of its
 * component.  Components are numbered 0 .. C-1 in ascending order of their smallest vertex id.  vertex_component[V] and
 * component_faces[C] (uint32) are a function of (V, faces) alone: of no arrival order, launch geometry or earlier call.
 *
 * Filter.  min_faces keeps the components with at least that many faces; largest keeps only the component with the most faces (ties:
 * the smaller component id), and min_faces still applies on top.  min_faces = 0, largest = 0 is the identity.  Kept faces keep their
 * order and winding with ids renumbered; a vertex is kept when its component is, and kept vertices keep their order.  Positions,
 * normals and colours are copied as 32-bit words, NaN payloads included.  Outputs must not overlap inputs (KFX_E_RANGE).
 *
 * Calls.  n_verts = V, n_faces = T and the scratch are the same in all of them; faces must not change between them.
 *   kfx_mesh_components_scratch_bytes   bytes of scratch for (V, T) alone: 12 per vertex (its parent / smallest id of its component, the
 *                                       face count of the component it is the smallest vertex of, its id after the filter) plus 16 per
 *                                       256 vertices and 8 per 256 faces (scan partials and bases) plus 256, each array rounded up to
 *                                       256: 256 + 3 r256(4 V) + 4 r256(4 ceil(V / 256)) + 2 r256(4 ceil(T / 256)).  0 if (V, T) is refused.
 *   kfx_mesh_components_plan    labels the mesh; blocks until counts_out = {C, faces of the largest component} is in host memory
 *                               (one 128-byte read-back).
 *   kfx_mesh_components_emit    writes vertex_component[V] and component_faces[C]; counts: the plan's.  Optional for a caller that
 *                               only filters.
 *   kfx_mesh_filter_plan        decides what min_faces / largest keep and numbers it; blocks until out = {V', T'} is in host memory (one
 *                               128-byte read-back, after the one that checks the scratch).  May be called again on the same scratch
 *                               with other parameters, without relabelling.
 *   kfx_mesh_filter_emit        writes verts_out[V'][3], faces_out[T'][3] and, where both the input and the output are given,
 *                               norms_out[V'][3] and colors_out[V'][4]; kept: the last filter plan's {V', T'}.
 * The scratch is 256-byte aligned and the library never allocates.  Its header keeps a magic word, V, T and the stage reached; every
 * call after the plan reads them back and refuses a stale or foreign scratch, or counts that are not the plan's, with KFX_E_RANGE.
 *
 * Returns 0 or KFX_E_*, all of these before any HIP call: null pointers KFX_E_NULL; V = 0 with T > 0, 3T >= 2^32, V > 3T or outputs
 * that overlap inputs KFX_E_RANGE; too little scratch KFX_E_SHAPE; a misaligned scratch (256) or array (4) KFX_E_ALIGN.  T = 0 launches
 * nothing and returns zeros.  A face id >= V: the plan's first kernel reads `faces` alone and raises an error word in the scratch; no
 * later kernel indexes anything by a face id before it has tested that word, and the plan returns KFX_E_RANGE. */
#ifndef KFX_MESH_CLEAN_H
#define KFX_MESH_CLEAN_H

#include "kfx.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t kfx_mesh_components_scratch_bytes(unsigned long long n_verts, unsigned long long n_faces);
int kfx_mesh_components_plan(const unsigned* faces, unsigned long long n_faces, unsigned long long n_verts, void* scratch,
                             size_t scratch_bytes, unsigned long long counts_out[2], kfx_stream stream);
int kfx_mesh_components_emit(const void* scratch, size_t scratch_bytes, unsigned long long n_verts, unsigned long long n_faces,
                             const unsigned long long counts[2], unsigned* vertex_component, unsigned* component_faces, kfx_stream stream);
int kfx_mesh_filter_plan(void* scratch, size_t scratch_bytes, unsigned long long n_verts, unsigned long long n_faces, const unsigned* faces,
                         unsigned long long min_faces, int largest, unsigned long long out[2], kfx_stream stream);
int kfx_mesh_filter_emit(const void* scratch, size_t scratch_bytes, unsigned long long n_verts, unsigned long long n_faces,
                         const unsigned long long kept[2], const float* verts, const float* norms, const float* colors, const unsigned* faces,
                         float* verts_out, float* norms_out, float* colors_out, unsigned* faces_out, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_MESH_CLEAN_H */
