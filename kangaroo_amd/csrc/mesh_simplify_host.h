// mesh_simplify_host.h -- what mesh_simplify.hip (include/kfx_mesh_simplify.h) decides on the host before it launches anything: the
// grid parameters it accepts, how the scratch is carved from (V, T), the refusals of the arrays (the counts, the scratch and the
// overlap rules are mesh_clean_host.h's); and the rules of the clustering themselves -- the cell key and d2 of a vertex, the key of a
// face, and insert / look-up of the two open-addressing tables -- written once over a memory policy, so that the kernels run them on
// agent-scope atomics and scripts/mesh_simplify_host_check.cpp on a plain array under the host sanitizers.  No HIP in here.
#pragma once

#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/kfx_mesh_simplify.h"
#include "mesh_clean_host.h"

namespace kfx {

constexpr unsigned long long SIMPLIFY_MAGIC = 0x6b66784d536d7031ull;   // "kfxMSmp1"
constexpr unsigned long long SIMPLIFY_MIN_CAP = 64;                    // slots of the smallest table
constexpr unsigned long long SIMPLIFY_SINGLETON = 1ull << 63;          // flag bit of a singleton's key; the rest is its vertex id
constexpr unsigned long long SIMPLIFY_VEMPTY = ~0ull;                  // a free slot of the vertex table (no entry: d2 <= 0.75)
constexpr unsigned SIMPLIFY_FEMPTY = 0xffffffffu;                      // a free slot of the face table (3T < 2^32: no face id)
constexpr float SIMPLIFY_CELLS = 1048576.0f;                           // cell indices lie in [-2^20, 2^20): 21 bits an axis

// the header's 64-bit words
enum SimplifyWord {
    SIMPLIFY_W_MAGIC = 0, SIMPLIFY_W_VERTS, SIMPLIFY_W_FACES, SIMPLIFY_W_STAGE,   // read back and compared by the emit
    SIMPLIFY_W_ERROR,                                                             // SIMPLIFY_ERR_* bits raised on the device (CLEAN_W_ERROR's place)
    SIMPLIFY_W_KEPT_VERTS, SIMPLIFY_W_KEPT_FACES,                                 // V', T'
    SIMPLIFY_WORDS = 16                                                           // what a read-back copies: 128 bytes
};
enum { SIMPLIFY_STAGE_NONE = 0, SIMPLIFY_STAGE_PLANNED = 1 };
enum { SIMPLIFY_ERR_FACE_ID = 1, SIMPLIFY_ERR_PROBE = 2 };   // a face id >= V; a probe beyond its cap (a bug: never raised by a correct build)
// the kernels the two passes share (mesh_clean_device.h) find the error word and the face-id bit where the clean-up keeps them
static_assert((int)SIMPLIFY_W_ERROR == (int)CLEAN_W_ERROR && (int)SIMPLIFY_ERR_FACE_ID == (int)CLEAN_ERR_FACE_ID, "shared kernels");

// the smallest power of two >= max(n, SIMPLIFY_MIN_CAP)
inline unsigned long long simplify_pow2(unsigned long long n)
{
    unsigned long long c = SIMPLIFY_MIN_CAP;
    while (c < n) c <<= 1;
    return c;
}

// The scratch (offsets in bytes from its start; include/kfx_mesh_simplify.h states the sum):
//   hdr     256 bytes: SimplifyWord
//   vtab    uint64 per slot, vcap = p2(2 V) slots: d2 bits << 32 | vertex id of the best vertex seen of the slot's cell
//   ftab    uint32 per slot, fcap = p2(2 T) slots: the smallest face id seen of the slot's cluster triple
//   rep     uint32 per vertex: the representative of its cluster
//   used    uint32 per vertex: 1 if it is a representative a kept face refers to
//   remap   uint32 per vertex: a written representative's new id, CLEAN_DROPPED for every other vertex
//   fkeep   uint32 per face: 1 if it is kept
//   vpart, vbase   uint32 per block of 256 vertices: the written representatives in it, those before it
//   fpart, fbase   uint32 per block of 256 faces: the kept faces in it, those before it
struct SimplifyScratch {
    size_t hdr, vtab, ftab, rep, used, remap, fkeep, vpart, vbase, fpart, fbase, bytes;
    unsigned long long vcap, fcap, vblk, fblk;
};
inline SimplifyScratch simplify_scratch(unsigned long long n_verts, unsigned long long n_faces)
{
    SimplifyScratch s{};
    s.vcap = simplify_pow2(2 * n_verts);
    s.fcap = simplify_pow2(2 * n_faces);
    s.vblk = (n_verts + CLEAN_BLOCK - 1) / CLEAN_BLOCK;
    s.fblk = (n_faces + CLEAN_BLOCK - 1) / CLEAN_BLOCK;
    s.hdr = 0;
    s.vtab = 256;
    s.ftab = s.vtab + (size_t)(8 * s.vcap);
    s.rep = s.ftab + (size_t)(4 * s.fcap);
    s.used = s.rep + clean_round256(4 * n_verts);
    s.remap = s.used + clean_round256(4 * n_verts);
    s.fkeep = s.remap + clean_round256(4 * n_verts);
    s.vpart = s.fkeep + clean_round256(4 * n_faces);
    s.vbase = s.vpart + clean_round256(4 * s.vblk);
    s.fpart = s.vbase + clean_round256(4 * s.vblk);
    s.fbase = s.fpart + clean_round256(4 * s.fblk);
    s.bytes = s.fbase + clean_round256(4 * s.fblk);
    return s;
}

// the scratch of accepted counts: present, large enough, aligned to 256 bytes -- in that order (clean_check_scratch's)
inline CleanRefusal simplify_check_scratch(unsigned long long n_verts, unsigned long long n_faces, const void* scratch, size_t scratch_bytes)
{
    if (!scratch) return {KFX_E_NULL, "null scratch"};
    if (scratch_bytes < simplify_scratch(n_verts, n_faces).bytes) return {KFX_E_SHAPE, "scratch smaller than kfx_mesh_simplify_scratch_bytes()"};
    if ((uintptr_t)scratch & 255) return {KFX_E_ALIGN, "scratch not aligned to 256 bytes"};
    return {0, nullptr};
}

inline bool simplify_finite(float x) { return fabsf(x) <= FLT_MAX; }   // (false for a NaN)

// The grid: origin and 1 / cell.  cell finite and > 0, 1 / cell finite, origin finite.
struct SimplifyGrid {
    float o[3], inv;
};
inline CleanRefusal simplify_check_grid(const float* origin, float cell, SimplifyGrid* g)
{
    if (!origin) return {KFX_E_NULL, "null origin"};
    if (!simplify_finite(cell) || !(cell > 0.0f)) return {KFX_E_RANGE, "cell is not a finite length > 0"};
    const float inv = 1.0f / cell;
    if (!simplify_finite(inv)) return {KFX_E_RANGE, "1 / cell is not finite"};
    for (int k = 0; k < 3; ++k)
        if (!simplify_finite(origin[k])) return {KFX_E_RANGE, "origin is not finite"};
    if (g) *g = SimplifyGrid{{origin[0], origin[1], origin[2]}, inv};
    return {0, nullptr};
}

// the emit's optional map: aligned, and sharing no byte with an input, an output or the scratch
inline CleanRefusal simplify_check_map(const void* map, unsigned long long n_verts, unsigned long long n_faces, const unsigned long long* kept,
                                       const void* const in[4], const void* const out[4], const void* scratch, size_t scratch_bytes)
{
    static const unsigned words[4] = {3, 3, 4, 3};
    if (CleanRefusal r = clean_check_array(map, true); r.code) return r;
    const unsigned long long bytes = 4 * n_verts;
    for (int k = 0; k < 4; ++k) {
        if (clean_ranges_overlap(map, bytes, in[k], 4ull * words[k] * (k == 3 ? n_faces : n_verts))) return {KFX_E_RANGE, "vertex_cluster overlaps an input"};
        if (clean_ranges_overlap(map, bytes, out[k], 4ull * words[k] * (k == 3 ? kept[1] : kept[0]))) return {KFX_E_RANGE, "vertex_cluster overlaps an output"};
    }
    if (clean_ranges_overlap(map, bytes, scratch, scratch_bytes)) return {KFX_E_RANGE, "vertex_cluster overlaps the scratch"};
    return {0, nullptr};
}

// ---- the rules of the clustering ----

// A vertex's cluster key and the bits of its d2.  Key: 21 bits an axis, i_k + 2^20, x lowest -- 63 bits; a singleton's is its own id
// under the flag bit, its d2 is 0.  d2 lies in [0, 0.75]: as a non-negative float its bits order as it does.
struct SimplifyVertex {
    unsigned long long key;
    unsigned d2;
};
KFX_CLEAN_HD unsigned simplify_bits(float x)
{
    union { float f; unsigned u; } b;
    b.f = x;
    return b.u;
}
KFX_CLEAN_HD SimplifyVertex simplify_vertex(const float* p, const SimplifyGrid& g, unsigned id)
{
    unsigned long long key = 0;
    float t[3];
    for (int k = 0; k < 3; ++k) {
        const float q = (p[k] - g.o[k]) * g.inv;
        if (!(fabsf(q) <= FLT_MAX)) return {SIMPLIFY_SINGLETON | id, 0u};
        const float i = floorf(q);
        if (!(i >= -SIMPLIFY_CELLS && i < SIMPLIFY_CELLS)) return {SIMPLIFY_SINGLETON | id, 0u};
        key |= (unsigned long long)((int)i + 1048576) << (21 * k);
        t[k] = (q - i) - 0.5f;
    }
    const float d2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
    return {key, simplify_bits(d2)};
}
KFX_CLEAN_HD unsigned long long simplify_vertex_word(const SimplifyVertex& v, unsigned id) { return (unsigned long long)v.d2 << 32 | id; }

// A face's key: its three clusters (representatives' ids) in ascending order.  degenerate: two of them are equal.
struct SimplifyTriple {
    unsigned a, b, c;
    KFX_CLEAN_HD bool operator==(const SimplifyTriple& o) const { return a == o.a && b == o.b && c == o.c; }
    KFX_CLEAN_HD bool degenerate() const { return a == b || b == c; }
};
KFX_CLEAN_HD SimplifyTriple simplify_triple(unsigned x, unsigned y, unsigned z)
{
    unsigned t;
    if (x > y) { t = x; x = y; y = t; }
    if (y > z) { t = y; y = z; z = t; }
    if (x > y) { t = x; x = y; y = t; }
    return {x, y, z};
}

// where a key starts probing: a 64-bit finaliser (neighbouring cells, which is what a mesh holds, spread out)
KFX_CLEAN_HD unsigned long long simplify_mix(unsigned long long h)
{
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}
KFX_CLEAN_HD unsigned long long simplify_hash(unsigned long long key) { return simplify_mix(key); }
KFX_CLEAN_HD unsigned long long simplify_hash(const SimplifyTriple& t)
{
    return simplify_mix(simplify_mix((unsigned long long)t.a << 32 | t.b) ^ t.c);
}

// The tables.  A slot holds one WORD (vertex table: d2 bits << 32 | vertex id, 64 bits; face table: a face id, 32 bits), all ones
// when it is free.  The key of a slot is not stored: key_of(word) recomputes it from the entry the word names, and every word a slot
// ever holds has the same key -- a free slot is claimed by a compare-and-swap, and a claimed one changes only by a minimum with a
// word of its key.  So whatever a probe reads, however stale, names the slot's key or reads as free.
// MEM is how the slots are reached: load(s), cas(s, expected, desired) returning the value found, and min(s, word).
//
// insert: from the key's first slot onwards -- free: claim it (a lost claim continues with what it found there); the slot's key is
// the word's: lower it, done; another key: the next slot.  No step waits for another lane: each either finishes or moves on.  At most
// `cap` = mask + 1 probes; a table at most half full always has a free slot, so the cap is not reached -- it is tested all the same,
// and false is returned beyond it: a bug ends as an error code, not as a hang.
template <typename WORD, typename MEM, typename KEY, typename KEYOF>
KFX_CLEAN_HD bool simplify_insert(MEM& m, unsigned long long mask, const KEY& key, WORD word, const KEYOF& key_of)
{
    const WORD empty = (WORD)~(WORD)0;
    unsigned long long s = simplify_hash(key) & mask;
    for (unsigned long long k = 0; k <= mask; ++k, s = (s + 1) & mask) {
        WORD cur = m.load(s);
        if (cur == empty) {
            cur = m.cas(s, empty, word);
            if (cur == empty) return true;
        }
        if (key_of(cur) == key) {
            if (word < cur) m.min(s, word);   // (cur only falls: a word that is not below it changes nothing)
            return true;
        }
    }
    return false;
}

// look-up, once no lane inserts any more: the word of the key's slot, all ones if the key is in no slot (or the cap is passed)
template <typename WORD, typename MEM, typename KEY, typename KEYOF>
KFX_CLEAN_HD WORD simplify_find(const MEM& m, unsigned long long mask, const KEY& key, const KEYOF& key_of)
{
    const WORD empty = (WORD)~(WORD)0;
    unsigned long long s = simplify_hash(key) & mask;
    for (unsigned long long k = 0; k <= mask; ++k, s = (s + 1) & mask) {
        const WORD cur = m.load(s);
        if (cur == empty) return empty;
        if (key_of(cur) == key) return cur;
    }
    return empty;
}

// key_of for the vertex table: the cell of the vertex a word names
struct SimplifyVertexKeyOf {
    const float* verts;
    SimplifyGrid g;
    KFX_CLEAN_HD unsigned long long operator()(unsigned long long word) const
    {
        const unsigned id = (unsigned)word;
        return simplify_vertex(verts + 3 * (size_t)id, g, id).key;
    }
};
// key_of for the face table: the cluster triple of the face a word names
struct SimplifyFaceKeyOf {
    const unsigned* faces;
    const unsigned* rep;
    KFX_CLEAN_HD SimplifyTriple operator()(unsigned f) const
    {
        const unsigned* const id = faces + 3 * (size_t)f;
        return simplify_triple(rep[id[0]], rep[id[1]], rep[id[2]]);
    }
};

} // namespace kfx
