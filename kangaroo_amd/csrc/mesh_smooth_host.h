// mesh_smooth_host.h -- what mesh_smooth.hip (include/kfx_mesh_smooth.h) decides on the host before it launches anything: how the three
// scratches are carved from (V, T), the refusals of the arrays and of the smoothing's parameters (the counts and the overlap rules are
// mesh_clean_host.h's); and the per-vertex rules themselves -- the rank of a corner slot in its segment, the neighbour entries, the
// flags, one smoothing pass and one normal of a vertex -- written once over how the neighbour entries are reached, so that the kernels
// run them on device memory and scripts/mesh_smooth_host_check.cpp on plain arrays under the host sanitizers.  No HIP in here.
#pragma once

#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/kfx_mesh_smooth.h"
#include "mesh_clean_host.h"

namespace kfx {

constexpr unsigned long long SMOOTH_MAGIC = 0x6b66784d536d7431ull;   // "kfxMSmt1"
constexpr unsigned ADJ_WIDE = 64;   // a vertex with MORE incidences than this is ranked and flagged by a workgroup, not by single lanes

// the header's 64-bit words
enum SmoothWord {
    SMOOTH_W_MAGIC = 0, SMOOTH_W_VERTS, SMOOTH_W_FACES, SMOOTH_W_STAGE,
    SMOOTH_W_ERROR,    // SMOOTH_ERR_* bits raised on the device (CLEAN_W_ERROR's place)
    SMOOTH_W_TOTAL,    // the scan's total: 3T
    SMOOTH_W_WIDE,     // vertices with more than ADJ_WIDE incidences
    SMOOTH_WORDS = 16  // what a read-back copies: 128 bytes
};
enum { SMOOTH_ERR_FACE_ID = 1, SMOOTH_ERR_ADJ = 2 };   // a face id >= V; adjacency arrays that are not this mesh's
static_assert((int)SMOOTH_W_ERROR == (int)CLEAN_W_ERROR && (int)SMOOTH_ERR_FACE_ID == (int)CLEAN_ERR_FACE_ID, "shared kernels");

// The scratch of kfx_mesh_adjacency (offsets in bytes from its start; include/kfx_mesh_smooth.h states the sum):
//   hdr     256 bytes: SmoothWord
//   cnt     uint32 per vertex: its incidences; then the cursor of the fill, which runs from inc_start[v] to inc_start[v + 1]
//   tmp     uint32 per corner slot: the slots of every vertex's segment in arrival order
//   wide    uint32 per possible wide vertex (3T / 64 + 1): the vertices with more than ADJ_WIDE incidences, in arrival order
//   vpart, vbase   uint32 per block of 256 vertices: the incidences in it, those before it
struct AdjScratch {
    size_t hdr, cnt, tmp, wide, vpart, vbase, bytes;
    unsigned long long vblk, wide_cap;
};
inline AdjScratch adj_scratch(unsigned long long n_verts, unsigned long long n_faces)
{
    AdjScratch s{};
    s.vblk = (n_verts + CLEAN_BLOCK - 1) / CLEAN_BLOCK;
    s.wide_cap = 3 * n_faces / 64 + 1;
    s.hdr = 0;
    s.cnt = 256;
    s.tmp = s.cnt + clean_round256(4 * n_verts);
    s.wide = s.tmp + clean_round256(12 * n_faces);
    s.vpart = s.wide + clean_round256(4 * s.wide_cap);
    s.vbase = s.vpart + clean_round256(4 * s.vblk);
    s.bytes = s.vbase + clean_round256(4 * s.vblk);
    return s;
}
// The scratch of kfx_mesh_smooth: the header, the second position buffer, the neighbour table (two uint32 per incidence)
struct SmoothScratch {
    size_t hdr, buf, table, bytes;
};
inline SmoothScratch smooth_scratch(unsigned long long n_verts, unsigned long long n_faces)
{
    SmoothScratch s{};
    s.hdr = 0;
    s.buf = 256;
    s.table = s.buf + clean_round256(12 * n_verts);
    s.bytes = s.table + clean_round256(24 * n_faces);
    return s;
}
constexpr size_t NORMALS_SCRATCH_BYTES = 256;   // the header alone

// a scratch of `need` bytes: present, large enough, aligned to 256 bytes -- in that order (clean_check_scratch's)
inline CleanRefusal smooth_check_scratch(size_t need, const void* scratch, size_t scratch_bytes)
{
    if (!scratch) return {KFX_E_NULL, "null scratch"};
    if (scratch_bytes < need) return {KFX_E_SHAPE, "scratch smaller than its *_scratch_bytes()"};
    if ((uintptr_t)scratch & 255) return {KFX_E_ALIGN, "scratch not aligned to 256 bytes"};
    return {0, nullptr};
}

inline bool smooth_finite_host(float x) { return fabsf(x) <= FLT_MAX; }   // (false for a NaN)

// lambda in (0, 1], mu <= 0, both finite; iterations >= 0
inline CleanRefusal smooth_check_params(int iterations, float lambda, float mu)
{
    if (iterations < 0) return {KFX_E_RANGE, "iterations < 0"};
    if (!smooth_finite_host(lambda) || !smooth_finite_host(mu)) return {KFX_E_RANGE, "lambda or mu is not finite"};
    if (!(lambda > 0.0f && lambda <= 1.0f)) return {KFX_E_RANGE, "lambda outside (0, 1]"};
    if (mu > 0.0f) return {KFX_E_RANGE, "mu > 0"};
    return {0, nullptr};
}

// Arrays of 32-bit words with their sizes in bytes: each present (unless optional) and aligned to 4 bytes; no output shares a byte with
// an input, another output or the scratch.
struct SmoothArray {
    const void* p;
    unsigned long long bytes;
    bool optional;
};
inline CleanRefusal smooth_check_arrays(const SmoothArray* in, int n_in, const SmoothArray* out, int n_out, const void* scratch, size_t scratch_bytes)
{
    for (int k = 0; k < n_in; ++k)
        if (CleanRefusal r = clean_check_array(in[k].p, in[k].optional); r.code) return r;
    for (int k = 0; k < n_out; ++k)
        if (CleanRefusal r = clean_check_array(out[k].p, out[k].optional); r.code) return r;
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (clean_ranges_overlap(out[o].p, out[o].bytes, in[i].p, in[i].bytes)) return {KFX_E_RANGE, "an output overlaps an input"};
        for (int p = o + 1; p < n_out; ++p)
            if (clean_ranges_overlap(out[o].p, out[o].bytes, out[p].p, out[p].bytes)) return {KFX_E_RANGE, "two outputs overlap"};
        if (clean_ranges_overlap(out[o].p, out[o].bytes, scratch, scratch_bytes)) return {KFX_E_RANGE, "an output overlaps the scratch"};
    }
    for (int i = 0; i < n_in; ++i)
        if (clean_ranges_overlap(in[i].p, in[i].bytes, scratch, scratch_bytes)) return {KFX_E_RANGE, "the scratch overlaps an input"};
    return {0, nullptr};
}

// ---- the per-vertex rules ----

KFX_CLEAN_HD float smooth_float(unsigned u)
{
    union { float f; unsigned u; } b;
    b.u = u;
    return b.f;
}
KFX_CLEAN_HD unsigned smooth_word(float x)
{
    union { float f; unsigned u; } b;
    b.f = x;
    return b.u;
}
KFX_CLEAN_HD bool smooth_finite(float x) { return fabsf(x) <= FLT_MAX; }

// the rank of corner slot s among the d slots of its segment, which are distinct: the smaller ones
KFX_CLEAN_HD unsigned adj_rank(const unsigned* slots, unsigned d, unsigned s)
{
    unsigned rank = 0;
    for (unsigned j = 0; j < d; ++j) rank += slots[j] < s ? 1u : 0u;
    return rank;
}

// How the neighbour entries of one vertex are reached: at(k), k < 2 d.
// ... through the faces: entry 2 i is the corner after incidence i's, entry 2 i + 1 the corner after that
struct NbrFromFaces {
    const unsigned* faces;
    const unsigned* slots;   // the vertex's segment
    KFX_CLEAN_HD unsigned at(unsigned k) const
    {
        const unsigned s = slots[k >> 1], f = s / 3, c = s - 3 * f;
        const unsigned c1 = c + 1 + (k & 1);
        return faces[3 * (size_t)f + (c1 >= 3 ? c1 - 3 : c1)];
    }
};
// ... from a table that holds them as they come: two words per incidence
struct NbrFromTable {
    const unsigned* entries;   // the vertex's segment of the table
    KFX_CLEAN_HD unsigned at(unsigned k) const { return entries[k]; }
};

// The flag bits the neighbour entries first, first + step, ... of v's 2 d raise (BOUNDARY, NONMANIFOLD, DEGENERATE): the whole answer with
// (0, 1), a lane's share with (lane, lanes), to be OR-ed.  The counts do not depend on the order of the entries.
template <typename NBR>
KFX_CLEAN_HD unsigned adj_flags(const NBR& nbr, unsigned d, unsigned v, unsigned first, unsigned step)
{
    unsigned bits = 0;
    const unsigned n = 2 * d;
    for (unsigned i = first; i < n; i += step) {
        const unsigned u = nbr.at(i);
        if (u == v) {
            bits |= KFX_MESH_DEGENERATE;
            continue;
        }
        unsigned cnt = 0;
        for (unsigned j = 0; j < n; ++j) cnt += nbr.at(j) == u ? 1u : 0u;
        if (cnt == 1) bits |= KFX_MESH_BOUNDARY;
        if (cnt > 2) bits |= KFX_MESH_NONMANIFOLD;
    }
    return bits;
}

// One smoothing pass of vertex v: p the positions of the pass's input as 32-bit words, d its incidences, pinned: its flags meet the
// mask.  out: the three words of its row.
template <typename NBR>
KFX_CLEAN_HD void smooth_vertex(const unsigned* p, unsigned v, const NBR& nbr, unsigned d, bool pinned, float factor, unsigned out[3])
{
    const unsigned* const me = p + 3 * (size_t)v;
    out[0] = me[0]; out[1] = me[1]; out[2] = me[2];
    if (d == 0 || pinned) return;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    const unsigned n = 2 * d;
    for (unsigned k = 0; k < n; ++k) {
        const unsigned* const q = p + 3 * (size_t)nbr.at(k);
        acc[0] = acc[0] + smooth_float(q[0]);
        acc[1] = acc[1] + smooth_float(q[1]);
        acc[2] = acc[2] + smooth_float(q[2]);
    }
    const float m = (float)n;
    float o[3];
    for (int k = 0; k < 3; ++k) {
        const float pk = smooth_float(me[k]);
        const float dk = acc[k] / m - pk;
        o[k] = pk + factor * dk;
    }
    if (!(smooth_finite(o[0]) && smooth_finite(o[1]) && smooth_finite(o[2]))) return;
    out[0] = smooth_word(o[0]); out[1] = smooth_word(o[1]); out[2] = smooth_word(o[2]);
}

// The normal of a vertex with the d incidences `slots`: the sum of e2 x e1 over its faces, in order, normalised
KFX_CLEAN_HD void normal_vertex(const unsigned* p, const unsigned* faces, const unsigned* slots, unsigned d, float out[3])
{
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (unsigned i = 0; i < d; ++i) {
        const unsigned* const id = faces + 3 * (size_t)(slots[i] / 3);
        const unsigned *const q0 = p + 3 * (size_t)id[0], *const q1 = p + 3 * (size_t)id[1], *const q2 = p + 3 * (size_t)id[2];
        float e1[3], e2[3];
        for (int k = 0; k < 3; ++k) {
            e1[k] = smooth_float(q1[k]) - smooth_float(q0[k]);
            e2[k] = smooth_float(q2[k]) - smooth_float(q0[k]);
        }
        const float nx = e1[2] * e2[1] - e1[1] * e2[2];   // e2 x e1: the side the extraction's normals lie on
        const float ny = e1[0] * e2[2] - e1[2] * e2[0];
        const float nz = e1[1] * e2[0] - e1[0] * e2[1];
        acc[0] = acc[0] + nx;
        acc[1] = acc[1] + ny;
        acc[2] = acc[2] + nz;
    }
    const float l2 = (acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2];
    if (d == 0 || !smooth_finite(l2) || !(l2 > 0.0f)) {
        out[0] = out[1] = out[2] = 0.0f;
        return;
    }
    const float l = sqrtf(l2);
    out[0] = acc[0] / l; out[1] = acc[1] / l; out[2] = acc[2] / l;
}

} // namespace kfx
