// mesh_simplify_host_check.cpp -- the host side of the mesh simplification (kangaroo_amd/csrc/mesh_simplify_host.h) under the host
// sanitizers, on a machine without a device: the carving of the scratch from (V, T) -- every region inside the total, none overlapping,
// each large enough for what the kernels index in it (a host array of exactly that size is written at the first and last index, so an
// arithmetic slip is an out-of-bounds access the address sanitizer reports), both tables at most half full; the refusals of a scratch,
// of a grid and of the emit's map, each with its code; the key rules on the cases the header names (floorf at negative coordinates and
// on a boundary, the singletons, the d2 of a tie); and the table rules themselves -- simplify_insert and simplify_find, the very
// templates the kernels instantiate over agent-scope atomics -- over a plain array, single-threaded, and over the same array reached
// through the compiler's atomics by a few std::threads, the whole plan restated on the host and compared with a brute-force clustering.
// The kernels are not covered here (tests/test_gpu_mesh_simplify.py), nor the entry points (tests/test_abi_mesh_simplify_cpu.py).
//   g++ -std=c++17 -O1 -g -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -pthread
//       scripts/mesh_simplify_host_check.cpp -o mesh_simplify_host_check && ./mesh_simplify_host_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <thread>
#include <tuple>
#include <vector>

#include "../kangaroo_amd/csrc/mesh_simplify_host.h"

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
    } while (0)

using namespace kfx;
typedef unsigned long long u64;

static size_t r256(u64 n) { return (size_t)((n + 255) / 256 * 256); }
static u64 p2(u64 n)
{
    u64 c = 64;
    while (c < n) c *= 2;
    return c;
}

// the header's formula
static size_t formula(u64 v, u64 t)
{
    const u64 vblk = (v + 255) / 256, fblk = (t + 255) / 256;
    return 256 + 8 * p2(2 * v) + 4 * p2(2 * t) + 3 * r256(4 * v) + r256(4 * t) + 2 * r256(4 * vblk) + 2 * r256(4 * fblk);
}

static void check_layout(u64 v, u64 t, bool touch)
{
    CHECK(clean_check_counts(v, t).code == 0);
    const SimplifyScratch s = simplify_scratch(v, t);
    CHECK(s.bytes == formula(v, t));
    CHECK(s.vcap >= 2 * v && s.fcap >= 2 * t && (s.vcap & (s.vcap - 1)) == 0 && (s.fcap & (s.fcap - 1)) == 0);
    CHECK(s.vcap >= SIMPLIFY_MIN_CAP && s.fcap >= SIMPLIFY_MIN_CAP && (s.vcap == SIMPLIFY_MIN_CAP || s.vcap < 4 * v) && (s.fcap == SIMPLIFY_MIN_CAP || s.fcap < 4 * t));
    const size_t off[] = {s.hdr, s.vtab, s.ftab, s.rep, s.used, s.remap, s.fkeep, s.vpart, s.vbase, s.fpart, s.fbase, s.bytes};
    const u64 need[] = {8 * SIMPLIFY_WORDS, 8 * s.vcap, 4 * s.fcap, 4 * v, 4 * v, 4 * v, 4 * t, 4 * s.vblk, 4 * s.vblk, 4 * s.fblk, 4 * s.fblk};
    CHECK(s.hdr == 0 && s.vtab == 256);
    for (int k = 0; k < 11; ++k) CHECK(off[k] % 256 == 0 && off[k + 1] >= off[k] && off[k + 1] - off[k] >= need[k]);
    if (touch) {
        std::vector<unsigned char> scratch(s.bytes);
        const unsigned w = 7;
        for (int k = 1; k < 11; ++k)
            if (need[k]) {
                memcpy(&scratch.at(off[k]), &w, 4);
                memcpy(&scratch.at(off[k] + need[k] - 4), &w, 4);
            }
        const u64 word = SIMPLIFY_MAGIC;
        memcpy(&scratch.at(8 * (SIMPLIFY_WORDS - 1)), &word, 8);
    }
    // the scratch's refusals, in their order: null, short, misaligned
    unsigned char* const p = (unsigned char*)(((uintptr_t)1 << 20));
    CHECK(simplify_check_scratch(v, t, nullptr, s.bytes).code == KFX_E_NULL);
    CHECK(simplify_check_scratch(v, t, p, s.bytes - 1).code == KFX_E_SHAPE && simplify_check_scratch(v, t, p + 1, s.bytes - 1).code == KFX_E_SHAPE);
    for (const int o : {1, 4, 16, 128, 255}) CHECK(simplify_check_scratch(v, t, p + o, s.bytes + 256).code == KFX_E_ALIGN);
    CHECK(simplify_check_scratch(v, t, p, s.bytes).code == 0 && simplify_check_scratch(v, t, p + 256, s.bytes + 1).code == 0);
}

static void check_grid_refusals()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float o[3] = {0.25f, -3.0f, 7.0f};
    SimplifyGrid g;
    CHECK(simplify_check_grid(o, 0.5f, &g).code == 0 && g.inv == 2.0f && g.o[0] == 0.25f && g.o[1] == -3.0f && g.o[2] == 7.0f);
    CHECK(simplify_check_grid(nullptr, 0.5f, &g).code == KFX_E_NULL);
    for (const float cell : {0.0f, -0.0f, -1.0f, inf, -inf, nan, std::numeric_limits<float>::denorm_min()})
        CHECK(simplify_check_grid(o, cell, &g).code == KFX_E_RANGE);
    for (int k = 0; k < 3; ++k)
        for (const float bad : {inf, -inf, nan}) {
            float q[3] = {0, 0, 0};
            q[k] = bad;
            CHECK(simplify_check_grid(q, 0.5f, &g).code == KFX_E_RANGE);
        }
    // the map: optional, aligned, overlapping nothing
    unsigned char* const base = (unsigned char*)(((uintptr_t)1 << 24));
    const void* in[4] = {base, nullptr, nullptr, base + 0x10000};
    const void* out[4] = {base + 0x20000, nullptr, nullptr, base + 0x30000};
    const u64 kept[2] = {50, 80};
    const void* scratch = base + 0x40000;
    CHECK(simplify_check_map(nullptr, 100, 200, kept, in, out, scratch, 4096).code == 0);
    CHECK(simplify_check_map(base + 0x50000, 100, 200, kept, in, out, scratch, 4096).code == 0);
    CHECK(simplify_check_map(base + 0x50002, 100, 200, kept, in, out, scratch, 4096).code == KFX_E_ALIGN);
    CHECK(simplify_check_map(base + 1196, 100, 200, kept, in, out, scratch, 4096).code == KFX_E_RANGE);     // the last word of verts
    CHECK(simplify_check_map(base + 1200, 100, 200, kept, in, out, scratch, 4096).code == 0);
    CHECK(simplify_check_map(base + 0x10000 - 396, 100, 200, kept, in, out, scratch, 4096).code == KFX_E_RANGE);   // the first of faces
    CHECK(simplify_check_map(base + 0x20000 + 596, 100, 200, kept, in, out, scratch, 4096).code == KFX_E_RANGE);   // the last of verts_out
    CHECK(simplify_check_map(base + 0x20000 + 600, 100, 200, kept, in, out, scratch, 4096).code == 0);
    CHECK(simplify_check_map(base + 0x40000 + 4092, 100, 200, kept, in, out, scratch, 4096).code == KFX_E_RANGE);
}

static SimplifyVertex vertex_of(float x, float y, float z, const SimplifyGrid& g, unsigned id)
{
    const float p[3] = {x, y, z};
    return simplify_vertex(p, g, id);
}

static void check_key_rules()
{
    const SimplifyGrid g{{0, 0, 0}, 1.0f};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    auto cell = [](long x, long y, long z) { return (u64)(x + 1048576) | (u64)(y + 1048576) << 21 | (u64)(z + 1048576) << 42; };
    // floorf, not truncation; a vertex exactly on k * cell belongs to cell k
    CHECK(vertex_of(-0.25f, 0.5f, 0.5f, g, 0).key == cell(-1, 0, 0) && vertex_of(0.25f, 0.5f, 0.5f, g, 0).key == cell(0, 0, 0));
    CHECK(vertex_of(-1.0f, 2.0f, -3.0f, g, 0).key == cell(-1, 2, -3));
    CHECK(vertex_of(std::nextafterf(-1.0f, -2.0f), 0, 0, g, 0).key == cell(-2, 0, 0) && vertex_of(std::nextafterf(2.0f, 0.0f), 0, 0, g, 0).key == cell(1, 0, 0));
    // d2: the centre is 0, a corner 0.75, mirror images tie
    CHECK(vertex_of(0.5f, 0.5f, 0.5f, g, 0).d2 == 0 && vertex_of(1.0f, 2.0f, 3.0f, g, 0).d2 == simplify_bits(0.75f));
    CHECK(vertex_of(0.25f, 0.5f, 0.5f, g, 1).d2 == vertex_of(0.75f, 0.5f, 0.5f, g, 2).d2 && vertex_of(0.25f, 0.5f, 0.5f, g, 1).d2 == simplify_bits(0.0625f));
    CHECK(simplify_vertex_word(vertex_of(0.25f, 0.5f, 0.5f, g, 1), 1) < simplify_vertex_word(vertex_of(0.75f, 0.5f, 0.5f, g, 2), 2));
    CHECK(simplify_vertex_word(vertex_of(0.5f, 0.5f, 0.5f, g, 9), 9) < simplify_vertex_word(vertex_of(0.25f, 0.5f, 0.5f, g, 1), 1));
    // singletons: a NaN, an infinity, a cell index outside [-2^20, 2^20) -- on any axis
    for (int k = 0; k < 3; ++k)
        for (const float bad : {nan, inf, -inf, 1048576.0f, -1048576.5f, 3e38f}) {
            float p[3] = {0.5f, 0.5f, 0.5f};
            p[k] = bad;
            const SimplifyVertex v = simplify_vertex(p, g, 77);
            CHECK(v.key == (SIMPLIFY_SINGLETON | 77) && v.d2 == 0);
        }
    CHECK(vertex_of(1048575.5f, -1048576.0f, 0, g, 5).key == cell(1048575, -1048576, 0));
    const SimplifyGrid fine{{0, 0, 0}, 3e38f};   // q overflows to an infinity
    CHECK(vertex_of(2.0f, 0, 0, fine, 3).key == (SIMPLIFY_SINGLETON | 3) && vertex_of(0.0f, 0, 0, fine, 3).key == cell(0, 0, 0));
    // the face key: sorted, of any rotation or winding
    const SimplifyTriple t = simplify_triple(7, 3, 5);
    CHECK(t.a == 3 && t.b == 5 && t.c == 7 && !t.degenerate());
    for (const auto& p : {std::make_tuple(3u, 5u, 7u), std::make_tuple(5u, 7u, 3u), std::make_tuple(7u, 5u, 3u), std::make_tuple(5u, 3u, 7u)})
        CHECK(simplify_triple(std::get<0>(p), std::get<1>(p), std::get<2>(p)) == t);
    CHECK(simplify_triple(4, 9, 4).degenerate() && simplify_triple(9, 4, 4).degenerate() && simplify_triple(4, 4, 9).degenerate() && simplify_triple(4, 4, 4).degenerate());
}

// a table as a plain array: what AgentSlots is on the device.  A slot only ever falls, and a claimed one keeps its key.
template <typename WORD>
struct PlainTable {
    std::vector<WORD>& slots;
    WORD load(u64 s) const { return slots.at(s); }
    WORD cas(u64 s, WORD expected, WORD desired) const
    {
        const WORD found = slots.at(s);
        if (found == expected) {
            CHECK(expected == (WORD)~(WORD)0);   // only a free slot is claimed
            slots.at(s) = desired;
        }
        return found;
    }
    void min(u64 s, WORD word) const
    {
        CHECK(slots.at(s) != (WORD)~(WORD)0);
        slots.at(s) = std::min(slots.at(s), word);
    }
};
// the same array reached by several threads: the compiler's atomics on its words
template <typename WORD>
struct SharedTable {
    WORD* slots;
    u64 cap;
    WORD load(u64 s) const { CHECK(s < cap); return __atomic_load_n(slots + s, __ATOMIC_RELAXED); }
    WORD cas(u64 s, WORD expected, WORD desired) const
    {
        CHECK(s < cap);
        __atomic_compare_exchange_n(slots + s, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return expected;
    }
    void min(u64 s, WORD word) const
    {
        CHECK(s < cap);
        WORD cur = __atomic_load_n(slots + s, __ATOMIC_RELAXED);
        while (word < cur && !__atomic_compare_exchange_n(slots + s, &cur, word, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
};

struct Mesh {
    std::vector<float> verts;
    std::vector<unsigned> faces;
};
struct Result {
    std::vector<unsigned> rep, faces_out, vertex_cluster, written;
};

// the plan and the emit restated on the host over `threads` threads (0: the plain table, no atomics)
static Result run(const Mesh& m, const SimplifyGrid& g, int threads)
{
    const unsigned V = (unsigned)(m.verts.size() / 3), T = (unsigned)(m.faces.size() / 3);
    const SimplifyScratch s = simplify_scratch(V, T);
    std::vector<u64> vtab(s.vcap, SIMPLIFY_VEMPTY);
    std::vector<unsigned> ftab(s.fcap, SIMPLIFY_FEMPTY), rep(V), used(V, 0), fkeep(T, 0);
    const SimplifyVertexKeyOf vkey{m.verts.data(), g};
    const SimplifyFaceKeyOf fkey{m.faces.data(), rep.data()};
    auto over = [&](unsigned n, auto body) {   // body(i) for i in [0, n), interleaved over the threads
        if (threads == 0) {
            for (unsigned i = 0; i < n; ++i) body(i);
            return;
        }
        std::vector<std::thread> pool;
        for (int k = 0; k < threads; ++k)
            pool.emplace_back([&, k] { for (unsigned i = k; i < n; i += threads) body(i); });
        for (auto& th : pool) th.join();
    };
    PlainTable<u64> pv{vtab};
    SharedTable<u64> sv{vtab.data(), s.vcap};
    over(V, [&](unsigned v) {
        const SimplifyVertex me = simplify_vertex(m.verts.data() + 3 * (size_t)v, g, v);
        const u64 word = simplify_vertex_word(me, v);
        CHECK(threads ? simplify_insert<u64>(sv, s.vcap - 1, me.key, word, vkey) : simplify_insert<u64>(pv, s.vcap - 1, me.key, word, vkey));
    });
    for (unsigned v = 0; v < V; ++v) {
        const SimplifyVertex me = simplify_vertex(m.verts.data() + 3 * (size_t)v, g, v);
        const u64 word = simplify_find<u64>(pv, s.vcap - 1, me.key, vkey);
        CHECK(word != SIMPLIFY_VEMPTY);
        rep[v] = (unsigned)word;
    }
    PlainTable<unsigned> pf{ftab};
    SharedTable<unsigned> sf{ftab.data(), s.fcap};
    over(T, [&](unsigned f) {
        const SimplifyTriple me = fkey(f);
        if (me.degenerate()) return;
        CHECK(threads ? simplify_insert<unsigned>(sf, s.fcap - 1, me, f, fkey) : simplify_insert<unsigned>(pf, s.fcap - 1, me, f, fkey));
    });
    for (unsigned f = 0; f < T; ++f) {
        const SimplifyTriple me = fkey(f);
        fkeep[f] = !me.degenerate() && simplify_find<unsigned>(pf, s.fcap - 1, me, fkey) == f;
        if (fkeep[f]) used[me.a] = used[me.b] = used[me.c] = 1;
    }
    Result r;
    r.rep = rep;
    std::vector<unsigned> remap(V, CLEAN_DROPPED);
    for (unsigned v = 0; v < V; ++v)
        if (rep[v] == v && used[v]) {
            remap[v] = (unsigned)r.written.size();
            r.written.push_back(v);
        }
    for (unsigned v = 0; v < V; ++v) r.vertex_cluster.push_back(remap[rep[v]]);
    for (unsigned f = 0; f < T; ++f)
        if (fkeep[f])
            for (int k = 0; k < 3; ++k) r.faces_out.push_back(remap[rep[m.faces[3 * (size_t)f + k]]]);
    return r;
}

// the contract, brute force: clusters in a map, faces in a map
static Result brute(const Mesh& m, const SimplifyGrid& g)
{
    const unsigned V = (unsigned)(m.verts.size() / 3), T = (unsigned)(m.faces.size() / 3);
    std::map<u64, u64> best;
    std::vector<u64> key(V);
    for (unsigned v = 0; v < V; ++v) {
        const SimplifyVertex me = simplify_vertex(m.verts.data() + 3 * (size_t)v, g, v);
        key[v] = me.key;
        const u64 word = simplify_vertex_word(me, v);
        auto it = best.find(me.key);
        if (it == best.end() || word < it->second) best[me.key] = word;
    }
    Result r;
    for (unsigned v = 0; v < V; ++v) r.rep.push_back((unsigned)best[key[v]]);
    std::map<std::tuple<unsigned, unsigned, unsigned>, unsigned> first;
    std::vector<char> keep(T, 0), used(V, 0);
    for (unsigned f = 0; f < T; ++f) {
        unsigned c[3];
        for (int k = 0; k < 3; ++k) c[k] = r.rep[m.faces[3 * (size_t)f + k]];
        if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) continue;
        std::sort(c, c + 3);
        if (first.emplace(std::make_tuple(c[0], c[1], c[2]), f).second) {
            keep[f] = 1;
            used[c[0]] = used[c[1]] = used[c[2]] = 1;
        }
    }
    std::vector<unsigned> remap(V, CLEAN_DROPPED);
    for (unsigned v = 0; v < V; ++v)
        if (used[v]) {
            CHECK(r.rep[v] == v);
            remap[v] = (unsigned)r.written.size();
            r.written.push_back(v);
        }
    for (unsigned v = 0; v < V; ++v) r.vertex_cluster.push_back(remap[r.rep[v]]);
    for (unsigned f = 0; f < T; ++f)
        if (keep[f])
            for (int k = 0; k < 3; ++k) r.faces_out.push_back(remap[r.rep[m.faces[3 * (size_t)f + k]]]);
    return r;
}

static bool same(const Result& a, const Result& b)
{
    return a.rep == b.rep && a.faces_out == b.faces_out && a.vertex_cluster == b.vertex_cluster && a.written == b.written;
}

static unsigned rng_state = 12345;
static unsigned rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static Mesh random_mesh(unsigned V, unsigned T, unsigned cells)
{
    Mesh m;
    for (unsigned i = 0; i < 3 * V; ++i) m.verts.push_back((float)(rnd() % 100000) / 100000.0f * (float)cells - 0.5f * (float)cells);
    for (unsigned i = 0; i < 3 * T; ++i) m.faces.push_back(rnd() % V);
    return m;
}

static void check_tables()
{
    const SimplifyGrid g{{0, 0, 0}, 1.0f};
    // hand-made: two triangles across a cell face collapse; the mirror pair keeps the first; the tie goes to the smaller id
    {
        const Mesh m{{0.5f, 0.5f, 0.5f, 0.9f, 0.1f, 0.5f, 1.1f, 0.9f, 0.5f, 1.5f, 0.5f, 0.5f}, {0, 1, 2, 1, 3, 2}};
        const Result r = run(m, g, 0);
        CHECK((r.rep == std::vector<unsigned>{0, 0, 3, 3}) && r.faces_out.empty() && r.written.empty());
    }
    {
        const Mesh m{{0.5f, 0.5f, 0.5f, 1.5f, 0.5f, 0.5f, 0.5f, 1.5f, 0.5f, 0.6f, 1.6f, 0.5f, 1.6f, 0.6f, 0.5f, 0.6f, 0.6f, 0.5f}, {1, 2, 0, 3, 4, 5, 2, 1, 5}};
        const Result r = run(m, g, 0);
        CHECK((r.faces_out == std::vector<unsigned>{1, 2, 0}) && (r.vertex_cluster == std::vector<unsigned>{0, 1, 2, 2, 1, 0}));
    }
    {
        const Mesh m{{0.125f, 0.5f, 0.5f, 0.25f, 0.5f, 0.5f, 0.75f, 0.5f, 0.5f, 1.5f, 0.5f, 0.5f, 0.5f, 1.5f, 0.5f, 1.5f, 1.5f, 0.5f}, {0, 3, 4, 2, 3, 5}};
        const Result r = run(m, g, 0);
        CHECK((r.rep == std::vector<unsigned>{1, 1, 1, 3, 4, 5}) && (r.faces_out == std::vector<unsigned>{0, 1, 2, 0, 1, 3}));
    }
    // random meshes, a few singletons among them: the plain table, and 1, 3 and 4 threads, all equal the brute force
    for (const auto& shape : {std::make_tuple(255u, 400u, 5u), std::make_tuple(256u, 400u, 5u), std::make_tuple(257u, 1000u, 3u),
                              std::make_tuple(5000u, 9000u, 1u), std::make_tuple(20000u, 40000u, 17u), std::make_tuple(3000u, 5000u, 40u)}) {
        Mesh m = random_mesh(std::get<0>(shape), std::get<1>(shape), std::get<2>(shape));
        m.verts[3 * 7] = std::numeric_limits<float>::quiet_NaN();
        m.verts[3 * 11 + 1] = std::numeric_limits<float>::infinity();
        m.verts[3 * 13 + 2] = 4e6f;
        const Result want = brute(m, g);
        CHECK(same(run(m, g, 0), want));
        for (const int threads : {1, 3, 4}) CHECK(same(run(m, g, threads), want));
    }
}

int main()
{
    for (const u64 t : {1ull, 16ull, 32ull, 33ull, 85ull, 255ull, 256ull, 257ull, 4948ull, 70000ull})
        for (const u64 v : {1ull, 3ull, 32ull, 33ull, 255ull, 256ull, 257ull, 2480ull, 65536ull, 210000ull})
            if (v <= 3 * t) check_layout(v, t, true);
    check_layout(0, 0, true);
    check_layout(1170000, 2200000, false);
    check_layout(3ull * 1431655765ull, 1431655765ull, false);   // the largest mesh: 3T = 2^32 - 1
    check_grid_refusals();
    check_key_rules();
    check_tables();
    printf("mesh_simplify_host_check: ok\n");
    return 0;
}
