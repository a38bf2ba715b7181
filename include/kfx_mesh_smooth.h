/* kfx_mesh_smooth.h -- smoothing of an indexed mesh in device memory: per-vertex incidence lists in a fixed order, Laplacian / Taubin
 * passes over them, and per-vertex normals recomputed from the faces.  Same library (libkfx.so); the extraction calls, the clean-up
 * (kfx_mesh_clean.h) and the simplification (kfx_mesh_simplify.h) stay as they are.
 *
 * Input.  An indexed mesh as kfx_mesh_clean.h accepts it: verts[V][3], faces[T][3] of uint32 ids, V <= 3T < 2^32.
 *
 * (a) Incidence lists, kfx_mesh_adjacency.  A corner slot is s = 3 f + c: corner c of face f.  The incidences of vertex v are the corner
 *   slots with faces[f][c] == v, listed in ascending s: inc[inc_start[v] .. inc_start[v + 1]) -- the stable counting sort of the 3T
 *   corner slots by vertex id; inc_start[0] = 0, inc_start[V] = 3T.  A face that names v twice gives two entries.
 *   The neighbour entries of v are, per incidence in order, a = faces[f][(c + 1) % 3] then b = faces[f][(c + 2) % 3]: two per incidence.
 *   With cnt(v, u) the number of neighbour entries of v equal to u, vertex_flags[v] (optional) has
 *     bit 0  KFX_MESH_BOUNDARY      some u != v has cnt(v, u) == 1
 *     bit 1  KFX_MESH_NONMANIFOLD   some u != v has cnt(v, u) > 2
 *     bit 2  KFX_MESH_DEGENERATE    some neighbour entry of v equals v
 *     bit 3  KFX_MESH_ISOLATED      v has no incidence
 *   inc_start[V + 1], inc[3T] and vertex_flags[V] (uint32) are a function of (V, faces) alone: of no arrival order, launch geometry or
 *   earlier call.  The scratch is exempt.
 *
 * (b) Smoothing, kfx_mesh_smooth.  One iteration is a pass with factor lambda followed by a pass with factor mu; the second pass is
 *   skipped when mu == 0 (plain Laplacian smoothing; mu < 0 is Taubin's).  A pass computes every vertex v from the positions p of the
 *   pass's input; all arithmetic is fp32, every operation rounded on its own (the library is built with -ffp-contract=off):
 *     acc = (0, 0, 0);  for each neighbour entry u of v, in order:  acc_k = acc_k + p[u]_k;
 *     m = (float)(number of neighbour entries);  d_k = acc_k / m - p[v]_k;  o_k = p[v]_k + factor * d_k.
 *   The row of v is copied as three 32-bit words, unchanged, if v has no incidence, if vertex_flags[v] & pin_mask is not zero, or if any
 *   o_k is not finite: a NaN never travels, and no NaN payload has to be matched.  Passes alternate between verts_out and a buffer of the
 *   scratch; the last one lands in verts_out.  iterations == 0 copies the input.
 *
 * (c) Normals, kfx_mesh_vertex_normals.  Per incidence of v in order, with the face's own corners p0 = p[faces[f][0]], p1, p2:
 *     e1 = p1 - p0;  e2 = p2 - p0;
 *     n_x = e1_z * e2_y - e1_y * e2_z;  n_y = e1_x * e2_z - e1_z * e2_x;  n_z = e1_y * e2_x - e1_x * e2_y;   (each product and each
 *     difference rounded on its own);  acc_k = acc_k + n_k.
 *   l2 = (acc_x * acc_x + acc_y * acc_y) + acc_z * acc_z;  norms_out[v]_k = acc_k / sqrtf(l2), and (0, 0, 0) where l2 is not finite or
 *   not greater than 0, or where v has no incidence.  The sign: n is e2 x e1, the NEGATIVE of e1 x e2 -- the side the extraction's normals
 *   (the SDF gradient, pointing to where the distance grows: out of the surface) lie on for the faces the extraction writes, which
 *   wind clockwise seen from outside.  Decided on the oracle's indexed mesh of a sphere (tests/test_mesh_smooth_cpu.py).
 *
 * Calls.  n_verts = V, n_faces = T.  Every output size follows from (V, T); only an error word is read back (128 bytes, once per call).
 *   kfx_mesh_adjacency_scratch_bytes   256 + r256(4 V) + r256(12 T) + r256(4 (3T / 64 + 1)) + 2 r256(4 ceil(V / 256)), r256 rounding up
 *                                      to 256: the header; a counter per vertex; the corner slots in arrival order; the list of the
 *                                      vertices with more than 64 incidences, which are ranked by a workgroup each; scan partials and
 *                                      bases.  0 if (V, T) is refused.
 *   kfx_mesh_smooth_scratch_bytes      256 + r256(12 V) + r256(24 T): the header, the second position buffer, and a private table of the
 *                                      neighbour entries (8 bytes per incidence), so that no pass goes through `faces`.  0 if refused.
 *   kfx_mesh_vertex_normals_scratch_bytes   256: the header.  0 if (V, T) is refused.
 *   kfx_mesh_adjacency        writes inc_start, inc and, if given, vertex_flags.
 *   kfx_mesh_smooth           writes verts_out[V][3].  vertex_flags may be null when pin_mask == 0.
 *   kfx_mesh_vertex_normals   writes norms_out[V][3].
 * The scratch is the caller's, 256-byte aligned, and the library never allocates.  It carries nothing from one call to the next.
 *
 * Returns 0 or KFX_E_*, all of these before any HIP call, with the codes of kfx_mesh_clean.h: null pointers KFX_E_NULL; V = 0 with
 * T > 0, 3T >= 2^32, V > 3T, an output that overlaps an input, another output or the scratch, iterations < 0, a lambda or mu that is
 * not finite, lambda outside (0, 1] and mu > 0 KFX_E_RANGE; too little scratch KFX_E_SHAPE; a misaligned scratch (256) or array (4)
 * KFX_E_ALIGN.  T = 0 launches nothing and writes nothing.  A face id >= V: the first kernel of each call reads `faces` alone and raises
 * an error word in the scratch; every later kernel tests that word before it does anything, so nothing is written to the outputs, and
 * the call returns KFX_E_RANGE.  kfx_mesh_smooth and kfx_mesh_vertex_normals check the adjacency they are given the same way, before
 * anything is indexed by it: inc_start[0] == 0, inc_start ascending, inc_start[V] == 3T, every inc < 3T, and (the smoothing) every
 * incidence names its vertex; arrays that are zeroed or belong to another mesh are refused with KFX_E_RANGE, the outputs untouched.
 * No lane waits for another lane, and every loop is bounded by a count fixed before it starts. */
#ifndef KFX_MESH_SMOOTH_H
#define KFX_MESH_SMOOTH_H

#include "kfx.h"

#define KFX_MESH_BOUNDARY 1u
#define KFX_MESH_NONMANIFOLD 2u
#define KFX_MESH_DEGENERATE 4u
#define KFX_MESH_ISOLATED 8u

#ifdef __cplusplus
extern "C" {
#endif

size_t kfx_mesh_adjacency_scratch_bytes(unsigned long long n_verts, unsigned long long n_faces);
size_t kfx_mesh_smooth_scratch_bytes(unsigned long long n_verts, unsigned long long n_faces);
size_t kfx_mesh_vertex_normals_scratch_bytes(unsigned long long n_verts, unsigned long long n_faces);
int kfx_mesh_adjacency(const unsigned* faces, unsigned long long n_faces, unsigned long long n_verts, unsigned* inc_start, unsigned* inc,
                       unsigned* vertex_flags, void* scratch, size_t scratch_bytes, kfx_stream stream);
int kfx_mesh_smooth(const float* verts, const unsigned* faces, unsigned long long n_faces, unsigned long long n_verts,
                    const unsigned* inc_start, const unsigned* inc, const unsigned* vertex_flags, int iterations, float lambda, float mu,
                    unsigned pin_mask, float* verts_out, void* scratch, size_t scratch_bytes, kfx_stream stream);
int kfx_mesh_vertex_normals(const float* verts, const unsigned* faces, unsigned long long n_faces, unsigned long long n_verts,
                            const unsigned* inc_start, const unsigned* inc, float* norms_out, void* scratch, size_t scratch_bytes,
                            kfx_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* KFX_MESH_SMOOTH_H */
