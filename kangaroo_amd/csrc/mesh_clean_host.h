// mesh_clean_host.h -- what mesh_clean.hip (include/kfx_mesh_clean.h) decides on the host before it launches anything: which (V, T)
// are accepted, how the scratch is carved from them, the refusals of a scratch, of the arrays and of outputs that overlap inputs; and
// the labelling rules themselves -- find, unite, the flatten walk -- written once over a memory policy, so that the kernels run them
// on agent-scope atomics and scripts/mesh_clean_host_check.cpp on a plain array under the host sanitizers.  No HIP in here.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kfx_mesh_clean.h"

#if defined(__HIPCC__)
#define KFX_CLEAN_HD __host__ __device__ __forceinline__
#else
#define KFX_CLEAN_HD inline
#endif

namespace kfx {

constexpr unsigned CLEAN_BLOCK = 256;                               // vertices / faces per scan block: one per thread of a workgroup
constexpr unsigned long long CLEAN_MAX_IDS = 4294967296ull;         // 3T < 2^32: ids and corner offsets stay 32-bit
constexpr unsigned long long CLEAN_MAGIC = 0x6b66784d436c6e31ull;   // "kfxMCln1"
constexpr unsigned CLEAN_DROPPED = 0xffffffffu;                     // remap[] of a vertex the filter drops (V <= 3T < 2^32: no id)

// the header's 64-bit words
enum CleanWord {
    CLEAN_W_MAGIC = 0, CLEAN_W_VERTS, CLEAN_W_FACES, CLEAN_W_STAGE,   // read back and compared by every call after the plan
    CLEAN_W_ERROR,        // CLEAN_ERR_* bits raised on the device
    CLEAN_W_COMPONENTS,   // C
    CLEAN_W_BEST,         // max over components of faces << 32 | ~(smallest vertex id): the largest component, ties to the smaller id
    CLEAN_W_KEPT_VERTS, CLEAN_W_KEPT_FACES, CLEAN_W_MIN_FACES, CLEAN_W_LARGEST,   // the last filter plan's
    CLEAN_WORDS = 16      // what a read-back copies: 128 bytes
};
enum { CLEAN_STAGE_NONE = 0, CLEAN_STAGE_LABELLED = 1, CLEAN_STAGE_FILTERED = 2 };
enum { CLEAN_ERR_FACE_ID = 1, CLEAN_ERR_WALK = 2 };   // a face id >= V; a walk beyond its cap (a bug: never raised by a correct build)

struct CleanRefusal {
    int code;
    const char* rule;
};

inline size_t clean_round256(unsigned long long n) { return (size_t)((n + 255) / 256 * 256); }

// The scratch (offsets in bytes from its start; include/kfx_mesh_clean.h states the sum):
//   hdr     256 bytes: CleanWord
//   parent  uint32 per vertex: while uniting, a vertex of its component with a smaller-or-equal id; after the flatten, the smallest
//   cnt     uint32 per vertex: the faces of the component whose smallest vertex it is (others 0)
//   remap   uint32 per vertex: its id after the last filter plan, CLEAN_DROPPED if it is dropped
//   rpart, rbase   uint32 per block of 256 vertices: the roots in it, those before it
//   vpart, vbase   uint32 per block of 256 vertices: the kept vertices in it, those before it
//   fpart, fbase   uint32 per block of 256 faces: the kept faces in it, those before it
struct CleanScratch {
    size_t hdr, parent, cnt, remap, rpart, rbase, vpart, vbase, fpart, fbase, bytes;
    unsigned long long vblk, fblk;
};
inline CleanScratch clean_scratch(unsigned long long n_verts, unsigned long long n_faces)
{
    CleanScratch s{};
    s.vblk = (n_verts + CLEAN_BLOCK - 1) / CLEAN_BLOCK;
    s.fblk = (n_faces + CLEAN_BLOCK - 1) / CLEAN_BLOCK;
    s.hdr = 0;
    s.parent = 256;
    s.cnt = s.parent + clean_round256(4 * n_verts);
    s.remap = s.cnt + clean_round256(4 * n_verts);
    s.rpart = s.remap + clean_round256(4 * n_verts);
    s.rbase = s.rpart + clean_round256(4 * s.vblk);
    s.vpart = s.rbase + clean_round256(4 * s.vblk);
    s.vbase = s.vpart + clean_round256(4 * s.vblk);
    s.fpart = s.vbase + clean_round256(4 * s.vblk);
    s.fbase = s.fpart + clean_round256(4 * s.fblk);
    s.bytes = s.fbase + clean_round256(4 * s.fblk);
    return s;
}

// (V, T): faces without vertices, ids beyond 32 bits, more vertices than face corners (vertices without faces among them)
inline CleanRefusal clean_check_counts(unsigned long long n_verts, unsigned long long n_faces)
{
    if (n_faces && !n_verts) return {KFX_E_RANGE, "faces without vertices (V = 0, T > 0)"};
    if (n_faces >= (CLEAN_MAX_IDS + 2) / 3) return {KFX_E_RANGE, "3T >= 2^32 (32-bit ids)"};
    if (n_verts > 3 * n_faces) return {KFX_E_RANGE, n_faces ? "more vertices than face corners (V > 3T)" : "vertices without faces (V > 0, T = 0)"};
    return {0, nullptr};
}
// the scratch of accepted counts: present, large enough, aligned to 256 bytes -- in that order
inline CleanRefusal clean_check_scratch(unsigned long long n_verts, unsigned long long n_faces, const void* scratch, size_t scratch_bytes)
{
    if (!scratch) return {KFX_E_NULL, "null scratch"};
    if (scratch_bytes < clean_scratch(n_verts, n_faces).bytes) return {KFX_E_SHAPE, "scratch smaller than kfx_mesh_components_scratch_bytes()"};
    if ((uintptr_t)scratch & 255) return {KFX_E_ALIGN, "scratch not aligned to 256 bytes"};
    return {0, nullptr};
}
// counts a plan can have made: components of (V, T); kept vertices and faces of them
inline CleanRefusal clean_check_planned(unsigned long long n_verts, unsigned long long n_faces, const unsigned long long* counts, bool kept)
{
    if (!counts) return {KFX_E_NULL, "null counts"};
    if (counts[0] > n_verts || counts[1] > n_faces || (!kept && n_verts && !counts[0])) return {KFX_E_RANGE, "counts out of range"};
    return {0, nullptr};
}
// an array of 32-bit words: present (unless optional) and aligned to 4 bytes
inline CleanRefusal clean_check_array(const void* p, bool optional)
{
    if (!p) return optional ? CleanRefusal{0, nullptr} : CleanRefusal{KFX_E_NULL, "null array"};
    if ((uintptr_t)p & 3) return {KFX_E_ALIGN, "array not aligned to 4 bytes"};
    return {0, nullptr};
}
// whether [a, a + a_bytes) and [b, b + b_bytes) share a byte (an empty or absent range shares none)
inline bool clean_ranges_overlap(const void* a, unsigned long long a_bytes, const void* b, unsigned long long b_bytes)
{
    if (!a || !b || !a_bytes || !b_bytes) return false;
    const unsigned long long a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
// The arrays of a filter emit.  in[4] / out[4]: verts, norms, colors, faces; words[4] = 3, 3, 4, 3 per row; inputs have V (faces: T)
// rows, outputs V' (T') rows.  No output may share a byte with any input, with another output or with the scratch.
inline CleanRefusal clean_check_filter_arrays(unsigned long long n_verts, unsigned long long n_faces, const unsigned long long* kept,
                                              const void* const in[4], const void* const out[4], const void* scratch, size_t scratch_bytes)
{
    static const unsigned words[4] = {3, 3, 4, 3};
    for (int k = 0; k < 4; ++k) {
        const bool optional = k == 1 || k == 2;   // (an output of no rows may be absent too)
        if (CleanRefusal r = clean_check_array(in[k], optional); r.code) return r;
        if (CleanRefusal r = clean_check_array(out[k], optional || !kept[k == 3 ? 1 : 0]); r.code) return r;
    }
    unsigned long long in_bytes[4], out_bytes[4];
    for (int k = 0; k < 4; ++k) {
        in_bytes[k] = 4ull * words[k] * (k == 3 ? n_faces : n_verts);
        out_bytes[k] = 4ull * words[k] * (k == 3 ? kept[1] : kept[0]);
    }
    for (int o = 0; o < 4; ++o) {
        for (int i = 0; i < 4; ++i)
            if (clean_ranges_overlap(out[o], out_bytes[o], in[i], in_bytes[i])) return {KFX_E_RANGE, "an output overlaps an input"};
        for (int p = o + 1; p < 4; ++p)
            if (clean_ranges_overlap(out[o], out_bytes[o], out[p], out_bytes[p])) return {KFX_E_RANGE, "two outputs overlap"};
        if (clean_ranges_overlap(out[o], out_bytes[o], scratch, scratch_bytes)) return {KFX_E_RANGE, "an output overlaps the scratch"};
    }
    return {0, nullptr};
}

// whether the component whose smallest vertex is `root`, with `faces` faces, passes the filter; best: CLEAN_W_BEST
KFX_CLEAN_HD bool clean_keeps(unsigned root, unsigned faces, unsigned long long min_faces, int largest, unsigned long long best)
{
    return faces >= min_faces && (!largest || root == ~(unsigned)best);
}
KFX_CLEAN_HD unsigned long long clean_best_key(unsigned root, unsigned faces) { return (unsigned long long)faces << 32 | (unsigned)~root; }

// ---- labelling: a lock-free union-find over parent[V], the larger root hooked under the smaller ----
// MEM is how parent[] is reached: load(i), store(i, v) and cas(i, expected, desired), which returns the value it found at i (the link
// was made iff that is `expected`).  Invariants, whatever the interleaving of the lanes that run these at once:
//   I1  parent[x] <= x, always.
//   I2  parent[x] is a vertex of x's true component, always.
//   I3  a root (parent[x] == x) is linked only by a cas that expects the root itself; every other store goes to a vertex that has
//       been READ as a non-root -- and a non-root never becomes a root again -- and stores one of its ancestors.
// So whatever a walk reads, however stale, is an ancestor of where it stands (I1, I2: an old value of parent[x] is x itself or a
// vertex x was once linked below), a walk's conclusion "this is a root" is confirmed by the value the cas returns and by no second
// load, and every loop descends strictly in vertex id: it ends within `cap` = V steps without help from any other lane.  The caps are
// tested all the same, and a walk beyond one sets `bad` and leaves: a bug ends as an error code, not as a hang.

// from x down to a vertex that read as its own parent; halves the path as it goes
template <typename MEM>
KFX_CLEAN_HD unsigned clean_find(MEM& m, unsigned x, unsigned cap, bool& bad)
{
    unsigned p = m.load(x);
    for (unsigned steps = 0; p != x; ++steps) {
        if (p > x || steps >= cap) { bad = true; break; }
        const unsigned g = m.load(p);
        if (g < p) m.store(x, g);   // x has been read as a non-root; g is an ancestor of p, so of x (I3)
        x = p;
        p = g;
    }
    return x;
}

// a and b end in one tree
template <typename MEM>
KFX_CLEAN_HD void clean_unite(MEM& m, unsigned a, unsigned b, unsigned cap, bool& bad)
{
    unsigned ra = clean_find(m, a, cap, bad), rb = clean_find(m, b, cap, bad);
    for (unsigned steps = 0; ra != rb && !bad; ++steps) {
        if (steps >= cap) { bad = true; break; }
        const unsigned hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const unsigned found = m.cas(hi, hi, lo);
        if (found == hi) break;   // linked: hi was a root (I3); lo may have stopped being one meanwhile, it is of the component all the same
        // hi had been linked already, below found < hi: go on from there; max(ra, rb) has fallen
        ra = lo;
        rb = clean_find(m, found, cap, bad);
    }
}

// the root of x once no lane unites any more (lanes that flatten store roots over ancestors: both are ancestors)
template <typename MEM>
KFX_CLEAN_HD unsigned clean_root(MEM& m, unsigned x, unsigned cap, bool& bad)
{
    unsigned p = m.load(x);
    for (unsigned steps = 0; p != x; ++steps) {
        if (p > x || steps >= cap) { bad = true; break; }
        x = p;
        p = m.load(x);
    }
    return x;
}

} // namespace kfx
