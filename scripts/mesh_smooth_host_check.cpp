// mesh_smooth_host_check.cpp -- the host side of the mesh smoothing (kangaroo_amd/csrc/mesh_smooth_host.h) under the host sanitizers, on a
// machine without a device: the carving of the three scratches from (V, T) -- every region inside the total, none overlapping, each
// large enough for what the kernels index in it (a host array of exactly that size is written at the first and last index, so an
// arithmetic slip is an out-of-bounds access the address sanitizer reports); the refusals of a scratch, of the parameters and of the
// arrays, each with its code; and the per-vertex rules themselves -- adj_rank, adj_flags over both neighbour policies, smooth_vertex and
// normal_vertex, the very templates the kernels instantiate -- on plain arrays: the whole adjacency, a Taubin iteration and the normals
// restated on the host the way the kernels run them (segments filled in a scrambled order, then ranked) and compared with a naive
// reference of this file's own.
// The kernels are not covered here (tests/test_gpu_mesh_smooth.py), nor the entry points (tests/test_abi_mesh_smooth_cpu.py).
//   g++ -std=c++17 -O1 -g -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       scripts/mesh_smooth_host_check.cpp -o mesh_smooth_host_check && ./mesh_smooth_host_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "../kangaroo_amd/csrc/mesh_smooth_host.h"

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
    } while (0)

using namespace kfx;
typedef unsigned long long u64;

static size_t r256(u64 n) { return (size_t)((n + 255) / 256 * 256); }

static void check_layout(u64 v, u64 t, bool touch)
{
    CHECK(clean_check_counts(v, t).code == 0);
    const AdjScratch a = adj_scratch(v, t);
    const u64 vblk = (v + 255) / 256;
    CHECK(a.bytes == 256 + r256(4 * v) + r256(12 * t) + r256(4 * (3 * t / 64 + 1)) + 2 * r256(4 * vblk));
    CHECK(a.wide_cap * (ADJ_WIDE + 1) > 3 * t);   // more wide vertices than the list holds would need more than 3T incidences
    const size_t off[] = {a.hdr, a.cnt, a.tmp, a.wide, a.vpart, a.vbase, a.bytes};
    const u64 need[] = {8 * SMOOTH_WORDS, 4 * v, 12 * t, 4 * a.wide_cap, 4 * a.vblk, 4 * a.vblk};
    CHECK(a.hdr == 0 && a.cnt == 256 && a.vblk == vblk);
    for (int k = 0; k < 6; ++k) CHECK(off[k] % 256 == 0 && off[k + 1] >= off[k] && off[k + 1] - off[k] >= need[k]);
    const SmoothScratch s = smooth_scratch(v, t);
    CHECK(s.bytes == 256 + r256(12 * v) + r256(24 * t));
    CHECK(s.hdr == 0 && s.buf == 256 && s.table % 256 == 0 && s.table - s.buf >= 12 * v && s.bytes - s.table >= 24 * t);
    if (touch) {
        std::vector<unsigned char> scratch(a.bytes);
        for (int k = 0; k < 6; ++k)
            if (need[k]) scratch[off[k]] = scratch[off[k] + need[k] - 1] = 1;
        std::vector<unsigned char> second(s.bytes);
        if (v) second[s.buf] = second[s.buf + 12 * v - 1] = 1;
        if (t) second[s.table] = second[s.table + 24 * t - 1] = 1;
    }
}

static void check_refusals()
{
    alignas(256) static unsigned char block[1024];
    CHECK(smooth_check_scratch(512, nullptr, 512).code == KFX_E_NULL);
    CHECK(smooth_check_scratch(512, block, 511).code == KFX_E_SHAPE);
    CHECK(smooth_check_scratch(512, block + 4, 512).code == KFX_E_ALIGN);
    CHECK(smooth_check_scratch(512, block, 512).code == 0);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    CHECK(smooth_check_params(0, 0.5f, -0.53f).code == 0 && smooth_check_params(7, 1.0f, 0.0f).code == 0 && smooth_check_params(1, 0.5f, -0.0f).code == 0);
    CHECK(smooth_check_params(-1, 0.5f, -0.53f).code == KFX_E_RANGE);
    for (float bad : {0.0f, -0.5f, 1.0000001f, nan, inf, -inf}) CHECK(smooth_check_params(1, bad, -0.53f).code == KFX_E_RANGE);
    for (float bad : {0.01f, nan, inf, -inf}) CHECK(smooth_check_params(1, 0.5f, bad).code == KFX_E_RANGE);
    // arrays: an absent one, a misaligned one, an output on an input, on another output, on the scratch; the scratch on an input
    const unsigned char* const base = block;
    SmoothArray in[2] = {{base, 64, false}, {nullptr, 64, true}};
    SmoothArray out[2] = {{base + 128, 64, false}, {base + 192, 64, false}};
    const void* const scratch = base + 512;
    CHECK(smooth_check_arrays(in, 2, out, 2, scratch, 256).code == 0);
    in[1].optional = false;
    CHECK(smooth_check_arrays(in, 2, out, 2, scratch, 256).code == KFX_E_NULL);
    in[1] = {base + 66, 60, false};
    CHECK(smooth_check_arrays(in, 2, out, 2, scratch, 256).code == KFX_E_ALIGN);
    in[1] = {base + 64, 64, false};
    CHECK(smooth_check_arrays(in, 2, out, 2, scratch, 256).code == 0);
    out[0].p = base + 124;
    CHECK(smooth_check_arrays(in, 2, out, 2, scratch, 256).code == KFX_E_RANGE);
    out[0].p = base + 132;
    CHECK(smooth_check_arrays(in, 2, out, 2, scratch, 256).code == KFX_E_RANGE);
    out[0].p = base + 128;
    out[1].p = base + 508;
    CHECK(smooth_check_arrays(in, 2, out, 2, scratch, 256).code == KFX_E_RANGE);
    out[1].p = base + 192;
    CHECK(smooth_check_arrays(in, 2, out, 2, base + 0, 256).code == KFX_E_RANGE);
}

static unsigned rnd(unsigned& state)
{
    state = state * 1664525u + 1013904223u;
    return state >> 8;
}

// A mesh the way the kernels run it: count, scan, fill every segment in a scrambled order, rank into inc[]; flags by lanes' shares;
// then one Taubin iteration and the normals through the templates -- against a naive reference written without them.
static void check_rules(unsigned V, unsigned T, unsigned seed, unsigned hub_faces)
{
    unsigned state = seed;
    std::vector<unsigned> faces(3 * (size_t)T);
    for (unsigned f = 0; f < T; ++f)
        for (int c = 0; c < 3; ++c) faces[3 * f + c] = f < hub_faces && c == 1 ? 0u : rnd(state) % V;
    std::vector<float> verts(3 * (size_t)V);
    for (auto& x : verts) x = (float)(rnd(state) % 4096) / 4096.0f + (float)(rnd(state) % 7) * 1e-3f;
    if (V > 5) verts[3 * 5 + 1] = std::numeric_limits<float>::quiet_NaN();
    const unsigned* const bits = (const unsigned*)verts.data();

    // the kernels' way
    std::vector<unsigned> start(V + 1, 0), cursor(V), tmp(3 * (size_t)T), inc(3 * (size_t)T, 0xffffffffu), flags(V);
    for (unsigned id : faces) ++start[id + 1];
    for (unsigned v = 0; v < V; ++v) start[v + 1] += start[v];
    for (unsigned v = 0; v < V; ++v) cursor[v] = start[v];
    std::vector<unsigned> arrival(3 * (size_t)T);
    for (unsigned s = 0; s < 3 * T; ++s) arrival[s] = s;
    for (unsigned s = 3 * T; s > 1; --s) std::swap(arrival[s - 1], arrival[rnd(state) % s]);
    for (unsigned s : arrival) tmp[cursor[faces[s]]++] = s;
    for (unsigned s = 0; s < 3 * T; ++s) {
        const unsigned v = faces[s], a = start[v], d = start[v + 1] - a;
        const unsigned at = a + adj_rank(tmp.data() + a, d, s);
        CHECK(at < start[v + 1] && inc[at] == 0xffffffffu);
        inc[at] = s;
    }
    for (unsigned v = 0; v < V; ++v) {
        const unsigned a = start[v], d = start[v + 1] - a;
        unsigned whole = d ? adj_flags(NbrFromFaces{faces.data(), tmp.data() + a}, d, v, 0u, 1u) : (unsigned)KFX_MESH_ISOLATED, shares = d ? 0u : whole;
        for (unsigned lane = 0; lane < 7 && d; ++lane) shares |= adj_flags(NbrFromFaces{faces.data(), inc.data() + a}, d, v, lane, 7u);
        CHECK(whole == shares);   // (the order of the entries does not matter, nor how they are shared out)
        flags[v] = whole;
    }
    std::vector<unsigned> table(6 * (size_t)T);
    for (unsigned v = 0; v < V; ++v)
        for (unsigned i = start[v]; i < start[v + 1]; ++i) {
            const NbrFromFaces nbr{faces.data(), inc.data() + start[v]};
            table[2 * (size_t)i] = nbr.at(2 * (i - start[v]));
            table[2 * (size_t)i + 1] = nbr.at(2 * (i - start[v]) + 1);
        }

    // the naive way
    std::vector<std::vector<unsigned>> slots(V);
    for (unsigned s = 0; s < 3 * T; ++s) slots[faces[s]].push_back(s);
    for (unsigned v = 0; v < V; ++v) {
        CHECK(slots[v].size() == start[v + 1] - start[v]);
        CHECK(std::equal(slots[v].begin(), slots[v].end(), inc.begin() + start[v]));
        std::map<unsigned, unsigned> cnt;
        unsigned want = slots[v].empty() ? (unsigned)KFX_MESH_ISOLATED : 0u;
        std::vector<unsigned> entries;
        for (unsigned s : slots[v]) {
            const unsigned f = s / 3, c = s % 3;
            entries.push_back(faces[3 * f + (c + 1) % 3]);
            entries.push_back(faces[3 * f + (c + 2) % 3]);
        }
        for (unsigned u : entries) ++cnt[u];
        for (auto& kv : cnt) {
            if (kv.first == v) want |= KFX_MESH_DEGENERATE;
            else if (kv.second == 1) want |= KFX_MESH_BOUNDARY;
            else if (kv.second > 2) want |= KFX_MESH_NONMANIFOLD;
        }
        CHECK(flags[v] == want);
        CHECK(entries.size() == 2 * slots[v].size() && std::equal(entries.begin(), entries.end(), table.begin() + 2 * (size_t)start[v]));
        // one pass with each factor, pinned and not, through both policies
        for (float factor : {0.5f, -0.53f})
            for (unsigned pin : {0u, 1u}) {
                const bool pinned = (flags[v] & pin) != 0;
                unsigned got[3], again[3];
                smooth_vertex(bits, v, NbrFromTable{table.data() + 2 * (size_t)start[v]}, (unsigned)slots[v].size(), pinned, factor, got);
                smooth_vertex(bits, v, NbrFromFaces{faces.data(), inc.data() + start[v]}, (unsigned)slots[v].size(), pinned, factor, again);
                float o[3];
                bool moved = !entries.empty() && !pinned;
                for (int k = 0; k < 3 && moved; ++k) {
                    volatile float acc = 0.0f;
                    for (unsigned u : entries) acc = acc + verts[3 * (size_t)u + k];
                    volatile float mean = acc / (float)entries.size();
                    volatile float d = mean - verts[3 * (size_t)v + k];
                    volatile float step = factor * d;
                    o[k] = verts[3 * (size_t)v + k] + step;
                }
                moved = moved && std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]);
                for (int k = 0; k < 3; ++k) {
                    unsigned want_word;
                    if (moved) memcpy(&want_word, &o[k], 4);
                    else want_word = bits[3 * (size_t)v + k];
                    CHECK(got[k] == want_word && again[k] == want_word);
                }
            }
        // the normal
        float n[3];
        normal_vertex(bits, faces.data(), inc.data() + start[v], (unsigned)slots[v].size(), n);
        volatile float acc[3] = {0.0f, 0.0f, 0.0f};
        for (unsigned s : slots[v]) {
            const unsigned* const id = faces.data() + 3 * (size_t)(s / 3);
            volatile float e1[3], e2[3];
            for (int k = 0; k < 3; ++k) {
                e1[k] = verts[3 * (size_t)id[1] + k] - verts[3 * (size_t)id[0] + k];
                e2[k] = verts[3 * (size_t)id[2] + k] - verts[3 * (size_t)id[0] + k];
            }
            for (int k = 0; k < 3; ++k) {
                volatile float left = e1[(k + 2) % 3] * e2[(k + 1) % 3], right = e1[(k + 1) % 3] * e2[(k + 2) % 3];   // e2 x e1
                volatile float term = left - right;
                acc[k] = acc[k] + term;
            }
        }
        volatile float xx = acc[0] * acc[0], yy = acc[1] * acc[1], zz = acc[2] * acc[2];
        volatile float xy = xx + yy;
        volatile float l2 = xy + zz;
        const bool ok = !slots[v].empty() && std::isfinite(l2) && l2 > 0.0f;
        for (int k = 0; k < 3; ++k) {
            const float want_n = ok ? acc[k] / sqrtf(l2) : 0.0f;
            CHECK(memcmp(&want_n, &n[k], 4) == 0);
        }
    }
}

int main()
{
    const u64 counts[][2] = {{0, 0}, {1, 1}, {3, 1}, {255, 85}, {256, 86}, {257, 171}, {2480, 4948}, {1170000, 2200000}, {65536, 65536}};
    for (auto& c : counts) check_layout(c[0], c[1], c[1] < 100000);
    check_layout(3ull * 1431655764, 1431655764, false);   // the most faces: 3T < 2^32
    check_refusals();
    check_rules(3, 1, 1, 0);
    check_rules(40, 100, 2, 0);
    check_rules(257, 400, 3, 0);
    check_rules(300, 500, 4, 200);   // a hub of 200 faces among them: a wide vertex
    printf("mesh_smooth_host_check: ok\n");
    return 0;
}
