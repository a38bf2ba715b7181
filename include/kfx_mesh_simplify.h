/* kfx_mesh_simplify.h -- level of detail for an indexed mesh in device memory: vertex clustering on a world-anchored grid.  The one
 * stage of the mesh pipeline whose output is smaller than its input, so it runs before the download.  Same library (libkfx.so); the
 * extraction calls and the clean-up (kfx_mesh_clean.h) stay as they are.
 *
 * Input.  An indexed mesh as kfx_mesh_clean.h accepts it: verts[V][3], faces[T][3] of uint32 ids, V <= 3T < 2^32; norms[V][3] and
 * colors[V][4] are optional.  Parameters origin[3] and cell > 0, finite floats in world units.
 *
 * Cell of a vertex.  All arithmetic is fp32, every operation rounded on its own (the library is built with -ffp-contract=off).
 *   inv = 1.0f / cell, computed once on the host;  q_k = (p_k - origin_k) * inv;  i_k = floorf(q_k) -- floorf, not truncation: -0.25
 *   and +0.25 lie in different cells, and a vertex exactly on k * cell belongs to cell k.
 *   A vertex is a SINGLETON if any q_k is not finite or any i_k lies outside [-2^20, 2^20): a cluster of its own, never merged, its own
 *   representative.  All other vertices with equal (i_x, i_y, i_z) form one cluster.
 *
 * Representative.  t_k = (q_k - i_k) - 0.5f;  d2 = (t_x*t_x + t_y*t_y) + t_z*t_z;  the representative of a cluster is its vertex with
 * the smallest d2, ties to the smaller vertex id.  The cluster's output row is the representative's position, normal and colour, copied
 * as 32-bit words.  Nothing is averaged: a float sum depends on the order of arrival.
 *
 * Faces.  Every id is replaced by its cluster.  A face with two equal clusters is dropped.  Among the remaining faces with the same
 * unordered set of three clusters -- of any rotation or winding -- the one with the smallest input face id is kept, the rest are
 * dropped.  Kept faces keep their order and winding.
 *
 * Vertices out.  A cluster is written only if a kept face refers to it; written clusters are numbered in ascending order of their
 * representative's vertex id.  vertex_cluster[V] (optional) gives each input vertex's new id, 0xffffffff if its cluster is not written.
 *
 * Every output is a function of the inputs and (origin, cell) alone: of no arrival order, launch geometry or earlier call.  The scratch
 * is exempt: the slot a hash table gives an entry may differ from run to run.
 *
 * Calls.  n_verts = V, n_faces = T and the scratch are the same in both; verts and faces must not change between them.
 *   kfx_mesh_simplify_scratch_bytes   bytes of scratch for (V, T) alone.  With p2(n) the smallest power of two >= max(n, 64) and r256
 *                                     rounding up to 256:
 *                                       256 + 8 p2(2 V) + 4 p2(2 T) + 3 r256(4 V) + r256(4 T) + 2 r256(4 ceil(V / 256)) + 2 r256(4 ceil(T / 256))
 *                                     -- the header; a vertex table of 8-byte slots and a face table of 4-byte slots, each at most half
 *                                     full; per vertex its representative, a "referred to" flag and its new id; per face a "kept" flag;
 *                                     scan partials and bases.  0 if (V, T) is refused.
 *   kfx_mesh_simplify_plan   clusters the vertices, decides the faces and numbers what is kept; blocks until out = {V', T'} is in host
 *                            memory (one 128-byte read-back).
 *   kfx_mesh_simplify_emit   writes verts_out[V'][3], faces_out[T'][3], where both the input and the output are given norms_out[V'][3]
 *                            and colors_out[V'][4], and, if given, vertex_cluster[V]; kept: the plan's {V', T'}.
 * The scratch is 256-byte aligned and the library never allocates.  Its header keeps a magic word, V, T, the stage reached and an
 * error word; the emit reads them back and refuses a stale or foreign scratch, or counts that are not the plan's, with KFX_E_RANGE.
 *
 * Returns 0 or KFX_E_*, all of these before any HIP call, with the codes of kfx_mesh_clean.h: null pointers KFX_E_NULL; V = 0 with
 * T > 0, 3T >= 2^32, V > 3T, outputs that overlap inputs, each other or the scratch, a cell that is not finite or <= 0 (or so small
 * that 1 / cell is not finite) and an origin that is not finite KFX_E_RANGE; too little scratch KFX_E_SHAPE; a misaligned scratch (256)
 * or array (4) KFX_E_ALIGN.  T = 0 launches nothing and returns zeros.  A face id >= V: the plan's first kernel reads `faces` alone and
 * raises an error word in the scratch; no later kernel indexes anything by a face id before it has tested that word, and the plan
 * returns KFX_E_RANGE.  A probe sequence that passes its cap -- the table's capacity, which a table at most half full never reaches --
 * raises the error word too: the plan fails, nothing spins. */
#ifndef KFX_MESH_SIMPLIFY_H
#define KFX_MESH_SIMPLIFY_H

#include "kfx.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t kfx_mesh_simplify_scratch_bytes(unsigned long long n_verts, unsigned long long n_faces);
int kfx_mesh_simplify_plan(const float* verts, const unsigned* faces, unsigned long long n_faces, unsigned long long n_verts,
                           const float origin[3], float cell, void* scratch, size_t scratch_bytes, unsigned long long out[2],
                           kfx_stream stream);
int kfx_mesh_simplify_emit(const void* scratch, size_t scratch_bytes, unsigned long long n_verts, unsigned long long n_faces,
                           const unsigned long long kept[2], const float* verts, const float* norms, const float* colors,
                           const unsigned* faces, float* verts_out, float* norms_out, float* colors_out, unsigned* faces_out,
                           unsigned* vertex_cluster, kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_MESH_SIMPLIFY_H */
