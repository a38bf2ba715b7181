// mesh_clean_host_check.cpp -- the host side of the mesh clean-up (kangaroo_amd/csrc/mesh_clean_host.h) under the host sanitizers, on a
// machine without a device: which (V, T) are accepted; the carving of the scratch from them -- every region inside the total, none
// overlapping, each large enough for what the kernels index in it (a host array of exactly that size is written at the first and last
// index, so an arithmetic slip is an out-of-bounds access the address sanitizer reports); the refusals of a scratch, of the arrays and
// of outputs that overlap inputs, each with its code and in its order; and the labelling rules themselves -- clean_find, clean_unite,
// clean_root, the very templates the kernels instantiate over agent-scope atomics, here over a plain array -- with the flatten, rank,
// count and filter rules restated on the host, on small meshes with known answers and on random ones against a breadth-first search.
// The kernels are not covered here (tests/test_gpu_mesh_clean.py), nor the entry points (tests/test_abi_mesh_clean_cpu.py).
//   g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all scripts/mesh_clean_host_check.cpp
//       -o mesh_clean_host_check && ./mesh_clean_host_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../kangaroo_amd/csrc/mesh_clean_host.h"

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
    } while (0)

using namespace kfx;
typedef unsigned long long u64;

static size_t r256(u64 n) { return (size_t)((n + 255) / 256 * 256); }

// the header's formula
static size_t formula(u64 v, u64 t)
{
    const u64 vblk = (v + 255) / 256, fblk = (t + 255) / 256;
    return 256 + 3 * r256(4 * v) + 4 * r256(4 * vblk) + 2 * r256(4 * fblk);
}

static int check_layout(u64 v, u64 t, bool touch)
{
    CHECK(clean_check_counts(v, t).code == 0);
    const CleanScratch s = clean_scratch(v, t);
    CHECK(s.bytes == formula(v, t));
    CHECK(s.vblk * CLEAN_BLOCK >= v && (s.vblk == 0 || (s.vblk - 1) * CLEAN_BLOCK < v));
    CHECK(s.fblk * CLEAN_BLOCK >= t && (s.fblk == 0 || (s.fblk - 1) * CLEAN_BLOCK < t));
    const size_t off[] = {s.hdr, s.parent, s.cnt, s.remap, s.rpart, s.rbase, s.vpart, s.vbase, s.fpart, s.fbase, s.bytes};
    const u64 need[] = {8 * CLEAN_WORDS, 4 * v, 4 * v, 4 * v, 4 * s.vblk, 4 * s.vblk, 4 * s.vblk, 4 * s.vblk, 4 * s.fblk, 4 * s.fblk};
    CHECK(s.hdr == 0 && s.parent == 256);
    for (int k = 0; k < 10; ++k) CHECK(off[k] % 256 == 0 && off[k + 1] >= off[k] && off[k + 1] - off[k] >= need[k]);
    if (touch) {
        std::vector<unsigned char> scratch(s.bytes);
        const unsigned w = 7;
        for (int k = 1; k < 10; ++k)
            if (need[k]) {
                memcpy(&scratch.at(off[k]), &w, 4);
                memcpy(&scratch.at(off[k] + need[k] - 4), &w, 4);
            }
        const u64 word = CLEAN_MAGIC;
        memcpy(&scratch.at(8 * (CLEAN_WORDS - 1)), &word, 8);
    }
    // the scratch's refusals, in their order: null, short, misaligned
    unsigned char* const p = (unsigned char*)(((uintptr_t)1 << 20));
    CHECK(clean_check_scratch(v, t, nullptr, s.bytes).code == KFX_E_NULL);
    CHECK(clean_check_scratch(v, t, p, s.bytes - 1).code == KFX_E_SHAPE && clean_check_scratch(v, t, p + 1, s.bytes - 1).code == KFX_E_SHAPE);
    for (const int o : {1, 4, 16, 128, 255}) CHECK(clean_check_scratch(v, t, p + o, s.bytes + 256).code == KFX_E_ALIGN);
    CHECK(clean_check_scratch(v, t, p, s.bytes).code == 0 && clean_check_scratch(v, t, p + 256, s.bytes + 1).code == 0);
    return 1;
}

// parent[] as a plain array: what AgentParent is on the device
struct PlainParent {
    std::vector<unsigned>& parent;
    unsigned load(unsigned i) const { return parent.at(i); }
    void store(unsigned i, unsigned v) const
    {
        CHECK(v <= i && parent.at(i) != i);   // I1; only a vertex that is no root is stored to (I3)
        parent.at(i) = v;
    }
    unsigned cas(unsigned i, unsigned expected, unsigned desired) const
    {
        const unsigned found = parent.at(i);
        if (found == expected) {
            CHECK(expected == i && desired < i);   // I3: a root, linked below a smaller id (I1)
            parent.at(i) = desired;
        }
        return found;
    }
};

struct Labels {
    std::vector<unsigned> vertex_component, component_faces;
    unsigned long long best = 0;
};

// the plan and the components emit, restated: init, unite every face, flatten, count, rank
static Labels label(const std::vector<unsigned>& faces, unsigned n_verts)
{
    const size_t n_faces = faces.size() / 3;
    std::vector<unsigned> parent(n_verts), cnt(n_verts, 0);
    for (unsigned v = 0; v < n_verts; ++v) parent[v] = v;
    PlainParent m{parent};
    bool bad = false;
    for (size_t f = 0; f < n_faces; ++f) {
        const unsigned a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        CHECK(a < n_verts && b < n_verts && c < n_verts);
        if (a != b) clean_unite(m, a, b, n_verts, bad);
        if (b != c) clean_unite(m, b, c, n_verts, bad);
    }
    for (unsigned v = 0; v < n_verts; ++v) {
        const unsigned r = clean_root(m, v, n_verts, bad);
        if (r != v) m.store(v, r);
    }
    CHECK(!bad);
    for (unsigned v = 0; v < n_verts; ++v) CHECK(parent[v] <= v && parent[parent[v]] == parent[v]);
    for (size_t f = 0; f < n_faces; ++f) cnt[parent[faces[3 * f]]] += 1;
    Labels l;
    l.vertex_component.assign(n_verts, 0);
    for (unsigned v = 0; v < n_verts; ++v)
        if (parent[v] == v) {
            l.vertex_component[v] = (unsigned)l.component_faces.size();
            l.component_faces.push_back(cnt[v]);
            l.best = std::max(l.best, clean_best_key(v, cnt[v]));
        }
    for (unsigned v = 0; v < n_verts; ++v) l.vertex_component[v] = l.vertex_component[parent[v]];
    return l;
}

// the same by breadth-first search over an adjacency list: components in ascending order of their smallest vertex
static Labels label_bfs(const std::vector<unsigned>& faces, unsigned n_verts)
{
    std::vector<std::vector<unsigned>> adj(n_verts);
    for (size_t f = 0; f < faces.size() / 3; ++f)
        for (int k = 0; k < 3; ++k) {
            adj[faces[3 * f + k]].push_back(faces[3 * f + (k + 1) % 3]);
            adj[faces[3 * f + (k + 1) % 3]].push_back(faces[3 * f + k]);
        }
    Labels l;
    const unsigned none = 0xffffffffu;
    l.vertex_component.assign(n_verts, none);
    for (unsigned v = 0; v < n_verts; ++v) {
        if (l.vertex_component[v] != none) continue;
        const unsigned id = (unsigned)l.component_faces.size();
        l.component_faces.push_back(0);
        std::vector<unsigned> queue{v};
        l.vertex_component[v] = id;
        for (size_t q = 0; q < queue.size(); ++q)
            for (const unsigned w : adj[queue[q]])
                if (l.vertex_component[w] == none) {
                    l.vertex_component[w] = id;
                    queue.push_back(w);
                }
    }
    for (size_t f = 0; f < faces.size() / 3; ++f) l.component_faces[l.vertex_component[faces[3 * f]]] += 1;
    return l;
}

static void check_mesh(const std::vector<unsigned>& faces, unsigned n_verts, const std::vector<unsigned>* vc = nullptr,
                       const std::vector<unsigned>* cf = nullptr)
{
    const Labels a = label(faces, n_verts), b = label_bfs(faces, n_verts);
    CHECK(a.vertex_component == b.vertex_component && a.component_faces == b.component_faces);
    if (vc) CHECK(a.vertex_component == *vc);
    if (cf) CHECK(a.component_faces == *cf);
    // the largest component: the most faces, ties to the smaller id -- and what the filter keeps
    if (!a.component_faces.empty()) {
        const size_t arg = std::max_element(a.component_faces.begin(), a.component_faces.end()) - a.component_faces.begin();   // (the first of equals)
        CHECK((unsigned)(a.best >> 32) == a.component_faces[arg]);
        unsigned root = 0;
        while (a.vertex_component[root] != arg) ++root;
        CHECK(~(unsigned)a.best == root);
        CHECK(clean_keeps(root, a.component_faces[arg], 0, 1, a.best) && clean_keeps(root, a.component_faces[arg], a.component_faces[arg], 1, a.best));
        CHECK(!clean_keeps(root, a.component_faces[arg], (u64)a.component_faces[arg] + 1, 1, a.best));
        CHECK(!clean_keeps(root + 1, a.component_faces[arg], 0, 1, a.best) && clean_keeps(root + 1, 5, 5, 0, a.best) && !clean_keeps(root + 1, 4, 5, 0, a.best));
    }
}

static unsigned rnd(unsigned& state)
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

int main()
{
    // (V, T): 3T < 2^32, V <= 3T
    const u64 tmax = 4294967295ull / 3;
    CHECK(clean_check_counts(0, 0).code == 0 && clean_check_counts(3, 1).code == 0 && clean_check_counts(3 * tmax, tmax).code == 0);
    CHECK(clean_check_counts(1, 0).code == KFX_E_RANGE && clean_check_counts(4, 1).code == KFX_E_RANGE && clean_check_counts(0, 5).code == KFX_E_RANGE);
    CHECK(clean_check_counts(1, tmax + 1).code == KFX_E_RANGE && clean_check_counts(1, ~0ull).code == KFX_E_RANGE && clean_check_counts(~0ull, 5).code == KFX_E_RANGE);
    CHECK(3 * tmax < CLEAN_MAX_IDS && 3 * (tmax + 1) >= CLEAN_MAX_IDS);

    int layouts = 0;
    for (const u64 t : {1ull, 2ull, 85ull, 86ull, 255ull, 256ull, 257ull, 4948ull, 70000ull, 2200000ull, tmax})
        for (const u64 v : {1ull, 3ull, 255ull, 256ull, 257ull, 2480ull, 1170000ull, 3 * tmax})
            if (v <= 3 * t) layouts += check_layout(v, t, v <= 70000 && t <= 70000);
    layouts += check_layout(0, 0, true);
    CHECK(clean_scratch(0, 0).bytes == 256 && clean_scratch(3, 1).bytes == 256 + 3 * 256 + 4 * 256 + 2 * 256);
    // about 12 bytes per vertex, next to nothing per face
    const double per_vertex = (double)clean_scratch(1170000, 2200000).bytes / 1170000;
    CHECK(per_vertex > 12.0 && per_vertex < 12.2);
    for (u64 n = 1; n < 3000; ++n) {
        CHECK(clean_scratch(n, 3000).bytes <= clean_scratch(n + 1, 3000).bytes);
        CHECK(clean_scratch(3, n).bytes <= clean_scratch(3, n + 1).bytes);
    }

    // counts a plan can have made
    const u64 ok[2] = {3, 100}, many[2] = {11, 100}, faces_over[2] = {3, 101}, none[2] = {0, 0};
    CHECK(clean_check_planned(10, 100, nullptr, false).code == KFX_E_NULL && clean_check_planned(10, 100, ok, false).code == 0);
    CHECK(clean_check_planned(10, 100, many, false).code == KFX_E_RANGE && clean_check_planned(10, 100, faces_over, true).code == KFX_E_RANGE);
    CHECK(clean_check_planned(10, 100, none, false).code == KFX_E_RANGE && clean_check_planned(10, 100, none, true).code == 0);

    // arrays: present (unless optional), aligned to 4
    const char* const p = (const char*)((uintptr_t)1 << 20);
    CHECK(clean_check_array(nullptr, false).code == KFX_E_NULL && clean_check_array(nullptr, true).code == 0);
    CHECK(clean_check_array(p + 2, true).code == KFX_E_ALIGN && clean_check_array(p + 4, false).code == 0);
    // ranges
    CHECK(clean_ranges_overlap(p, 16, p + 15, 1) && !clean_ranges_overlap(p, 16, p + 16, 16) && clean_ranges_overlap(p + 4, 4, p, 100));
    CHECK(!clean_ranges_overlap(p, 0, p, 16) && !clean_ranges_overlap(nullptr, 16, p, 16) && !clean_ranges_overlap(p, 16, p - 16, 16));
    // the arrays of a filter emit: V = 10, T = 8, V' = 6, T' = 4; rows of 12, 12, 16 and 12 bytes
    {
        const u64 kept[2] = {6, 4}, nothing[2] = {0, 0}, no_faces[2] = {6, 0};
        const char* const scratch = p + (1 << 16);
        const void* in[4] = {p, p + 120, p + 240, p + 400};
        const void* out[4] = {p + 1000, p + 1072, p + 1144, p + 1240};
        auto verdict = [&](const void* const* i, const void* const* o, const u64* k) { return clean_check_filter_arrays(10, 8, k, i, o, scratch, 4096).code; };
        CHECK(verdict(in, out, kept) == 0);
        const void* no_opt[4] = {p, nullptr, nullptr, p + 400};
        const void* out_no_opt[4] = {p + 1000, nullptr, nullptr, p + 1240};
        CHECK(verdict(no_opt, out_no_opt, kept) == 0 && verdict(no_opt, out, kept) == 0 && verdict(in, out_no_opt, kept) == 0);
        for (int k : {0, 3}) {
            const void* a[4] = {in[0], in[1], in[2], in[3]};
            const void* b[4] = {out[0], out[1], out[2], out[3]};
            a[k] = nullptr;
            CHECK(verdict(a, out, kept) == KFX_E_NULL);
            b[k] = nullptr;
            CHECK(verdict(in, b, kept) == KFX_E_NULL);
            CHECK(verdict(in, b, nothing) == 0);   // an output of no rows may be absent
        }
        const void* faceless[4] = {out[0], out[1], out[2], nullptr};
        CHECK(verdict(in, faceless, no_faces) == 0 && verdict(in, faceless, kept) == KFX_E_NULL);
        for (int k = 0; k < 4; ++k) {
            const void* a[4] = {in[0], in[1], in[2], in[3]};
            const void* b[4] = {out[0], out[1], out[2], out[3]};
            a[k] = (const char*)a[k] + 2;
            CHECK(verdict(a, out, kept) == KFX_E_ALIGN);
            b[k] = (const char*)b[k] + 1;
            CHECK(verdict(in, b, kept) == KFX_E_ALIGN);
        }
        // in place, the last byte of an input, the next output, the scratch: refused; exactly adjacent: accepted
        const void* in_place[4] = {in[0], out[1], out[2], out[3]};
        const void* last_byte[4] = {out[0], (const char*)in[3] + 92, out[2], out[3]};
        const void* on_next[4] = {out[0], out[1], (const char*)out[3] - 92, out[3]};
        const void* in_scratch[4] = {out[0], out[1], out[2], scratch + 4092};
        const void* adjacent[4] = {(const char*)in[0] - 72, out[1], out[2], (const char*)in[3] + 96};
        CHECK(verdict(in, in_place, kept) == KFX_E_RANGE && verdict(in, last_byte, kept) == KFX_E_RANGE && verdict(in, on_next, kept) == KFX_E_RANGE);
        CHECK(verdict(in, in_scratch, kept) == KFX_E_RANGE && verdict(in, adjacent, kept) == 0);
    }

    // hand-made meshes with known answers
    {
        const std::vector<unsigned> one{0, 1, 2}, vc1{0, 0, 0}, cf1{1};
        check_mesh(one, 3, &vc1, &cf1);
        const std::vector<unsigned> shared{0, 1, 2, 2, 3, 4}, vc2{0, 0, 0, 0, 0}, cf2{2};
        check_mesh(shared, 5, &vc2, &cf2);
        const std::vector<unsigned> disjoint{3, 4, 5, 0, 1, 2}, vc3{0, 0, 0, 1, 1, 1}, cf3{1, 1};
        check_mesh(disjoint, 6, &vc3, &cf3);
        const std::vector<unsigned> isolated{0, 2, 4, 9, 7, 6}, vc4{0, 1, 0, 2, 0, 3, 4, 4, 5, 4}, cf4{1, 0, 0, 0, 1, 0};
        check_mesh(isolated, 10, &vc4, &cf4);
        const std::vector<unsigned> degenerate{0, 1, 2, 4, 4, 4, 5, 5, 3, 1, 1, 2}, vc5{0, 0, 0, 1, 2, 1}, cf5{2, 1, 1};
        check_mesh(degenerate, 6, &vc5, &cf5);
    }
    // strips: ids ascending, descending (the deepest trees min-hooking can build) and shuffled; a fan around one hub
    int meshes = 5;
    for (const int order : {0, 1, 2}) {
        const unsigned n = 3000;
        std::vector<unsigned> id(n + 2), faces;
        for (unsigned i = 0; i < n + 2; ++i) id[i] = order == 1 ? n + 1 - i : i;
        unsigned state = 99;
        if (order == 2)
            for (unsigned i = n + 1; i > 0; --i) std::swap(id[i], id[rnd(state) % (i + 1)]);
        for (unsigned i = 0; i < n; ++i) faces.insert(faces.end(), {id[i], id[i + 1], id[i + 2]});
        const std::vector<unsigned> vc(n + 2, 0), cf{n};
        check_mesh(faces, n + 2, &vc, &cf);
        ++meshes;
    }
    {
        std::vector<unsigned> faces;
        for (unsigned i = 0; i < 4096; ++i) faces.insert(faces.end(), {4097u, i, i + 1});
        const std::vector<unsigned> vc(4098, 0), cf{4096};
        check_mesh(faces, 4098, &vc, &cf);
        ++meshes;
    }
    // random face lists, sparse to dense, against the breadth-first search
    unsigned state = 12345;
    for (int round = 0; round < 200; ++round) {
        const unsigned n_verts = 3 + rnd(state) % 400, n_faces = std::max(1u + rnd(state) % (n_verts * 2), (n_verts + 2) / 3);
        std::vector<unsigned> faces(3 * (size_t)n_faces);
        const unsigned span = 1 + rnd(state) % n_verts;   // faces of nearby ids: many components
        for (unsigned f = 0; f < n_faces; ++f) {
            const unsigned at = rnd(state) % n_verts;
            for (int k = 0; k < 3; ++k) faces[3 * f + k] = (at + rnd(state) % span) % n_verts;
        }
        check_mesh(faces, n_verts);
        ++meshes;
    }
    // a walk beyond its cap ends with `bad`, not for ever: a parent[] that breaks I1 (a cycle no build can make)
    {
        std::vector<unsigned> parent{1, 0, 2};
        struct Raw {
            std::vector<unsigned>& p;
            unsigned load(unsigned i) const { return p.at(i); }
            void store(unsigned i, unsigned v) const { p.at(i) = v; }
            unsigned cas(unsigned i, unsigned e, unsigned d) const { const unsigned f = p.at(i); if (f == e) p.at(i) = d; return f; }
        } m{parent};
        bool bad = false;
        clean_find(m, 0, 3, bad);
        CHECK(bad);
        bad = false;
        clean_root(m, 1, 3, bad);
        CHECK(bad);
        bad = false;
        clean_unite(m, 0, 2, 3, bad);
        CHECK(bad);
    }
    printf("mesh_clean_host_check: ok (%d layouts, %d meshes)\n", layouts, meshes);
    return 0;
}
