// raycast_bricks_host_check.cpp -- the host side of the brick ray-cast (kangaroo_amd/csrc/raycast_bricks_host.h) under the host
// sanitizers, on a machine without a device: which frames are accepted and their brick grid, the capacity rule of a table, the
// carving of the scratch from the brick counts -- every region inside the total, none overlapping -- the refusals of the counts, an
// id list and a scratch, each with its code and in its order, and a host model of the table: the kernels' own insert and look-up
// (the compare-and-swap a plain host one) on a host array of exactly the table's size, so a probe that left the table would be an
// out-of-bounds access the address sanitizer reports.  The id sets are adversarial: all ids congruent modulo the capacity, all ids
// hashing to one slot, n = 1, 255, 256, 257, ids at the frame's last brick, ids beyond the frame, repeated ids, a full table.
// The kernels are not covered here (tests/test_gpu_brick_raycast.py), nor the entry points (tests/test_abi_brick_raycast_cpu.py).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/raycast_bricks_host_check.cpp -o check && ./check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../kangaroo_amd/csrc/raycast_bricks_host.h"

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
    } while (0)

using namespace kfx;

static size_t r256(unsigned long long n) { return (size_t)((n + 255) / 256 * 256); }

// the header's formula
static unsigned long long cap_of(unsigned long long m)
{
    if (m == 0) return 0;
    unsigned long long c = 1;
    while (c < 2 * m) c <<= 1;
    return c;
}
static size_t formula(unsigned long long n, unsigned long long nc) { return 256 + r256(8 * cap_of(n)) + r256(8 * cap_of(nc)); }

static int check_counts(unsigned long long n, unsigned long long nc)
{
    const BrickRayScratch s = brick_ray_scratch(n, nc), grey = brick_ray_scratch(n, 0);
    CHECK(s.bytes == formula(n, nc) && grey.bytes == formula(n, 0));
    // the capacity rule: none for an empty list, else a power of two, at least 2 n and below 4 n, with its log2
    for (int k = 0; k < 2; ++k) {
        const BrickTable t = k ? s.ct : s.t;
        const unsigned long long m = k ? nc : n;
        CHECK(t.cap == cap_of(m));
        if (m == 0) { CHECK(t.cap == 0); continue; }
        CHECK(t.cap >= 2 && (t.cap & (t.cap - 1)) == 0 && t.cap >= 2 * m && t.cap < 4 * m && (1ull << t.log2cap) == t.cap && t.log2cap >= 1 && t.log2cap <= 32);
    }
    CHECK(s.hdr == 0 && s.tab == 256);
    for (const size_t off : {s.tab, s.ctab, s.bytes}) CHECK(off % 256 == 0);
    CHECK(s.ctab - s.tab >= 8 * s.t.cap && s.bytes - s.ctab >= 8 * s.ct.cap);
    // a grey layout is the front of the one with colour: the SDF table is where it was
    CHECK(grey.tab == s.tab && grey.bytes == s.ctab && grey.bytes <= s.bytes);
    // the scratch's refusals, in their order: null, short, misaligned
    unsigned char* const p = (unsigned char*)(((uintptr_t)1 << 20));
    CHECK(brick_ray_check_scratch(n, nc, nullptr, s.bytes).code == KFX_E_NULL);
    CHECK(brick_ray_check_scratch(n, nc, p, s.bytes - 1).code == KFX_E_SHAPE && brick_ray_check_scratch(n, nc, p + 1, s.bytes - 1).code == KFX_E_SHAPE);
    for (const int off : {1, 4, 16, 128, 255}) CHECK(brick_ray_check_scratch(n, nc, p + off, s.bytes + 256).code == KFX_E_ALIGN);
    CHECK(brick_ray_check_scratch(n, nc, p, s.bytes).code == 0 && brick_ray_check_scratch(n, nc, p + 256, s.bytes + 1).code == 0);
    return 1;
}

static unsigned host_cas(unsigned* word, unsigned expected, unsigned desired)
{
    const unsigned was = *word;
    if (was == expected) *word = desired;
    return was;
}

// Build the table of `ids` for a frame of nb bricks as the plan does (cleared, then every id below nb inserted with its list
// position) in an array of exactly its slots, and look up: every listed id of the frame at its position, every id of `absent` nowhere.
static int check_table(const std::vector<unsigned>& ids, unsigned nb, const std::vector<unsigned>& absent)
{
    const unsigned long long n = ids.size();
    const BrickTable t = brick_table(n);
    std::vector<unsigned> slots(2 * (size_t)t.cap, BRICK_SLOT_EMPTY);   // (the plan's memset: every word 0xffffffff)
    const BrickTableView view = brick_table_view(slots.data(), t, n);
    CHECK(n == 0 || (view.mask == t.cap - 1 && view.shift == 32 - t.log2cap && view.shift >= 0 && view.shift <= 31));
    for (unsigned i = 0; i < n; ++i) {
        CHECK(brick_slot_of(ids[i], view.shift) <= view.mask);
        if (ids[i] < nb) {
            const bool first = std::find(ids.begin(), ids.begin() + i, ids[i]) == ids.begin() + i;
            CHECK(brick_table_insert(slots.data(), view.mask, view.shift, ids[i], i, host_cas) == first);   // (a repeated id keeps its first entry)
        }
    }
    size_t used = 0;
    for (size_t k = 0; k < t.cap; ++k) used += slots[2 * k] != BRICK_SLOT_EMPTY;
    CHECK(used <= n && 2 * used <= t.cap);
    for (unsigned i = 0; i < n; ++i) {
        const int pos = brick_table_find(view, ids[i]);
        if (ids[i] >= nb) { CHECK(pos == -1); continue; }
        CHECK(pos >= 0 && (unsigned)pos < n && ids[(size_t)pos] == ids[i]);
        CHECK((unsigned)pos == (unsigned)(std::find(ids.begin(), ids.end(), ids[i]) - ids.begin()));
    }
    for (const unsigned id : absent)
        if (std::find(ids.begin(), ids.end(), id) == ids.end() || id >= nb) CHECK(brick_table_find(view, id) == -1);
    return 1;
}

static kfx_volume frame(size_t w, size_t h, size_t d)
{
    kfx_volume f{};
    f.w = w; f.h = h; f.d = d;   // (no storage: ptr and the pitches stay null / zero)
    for (int i = 0; i < 3; ++i) { f.boxmin[i] = -1.0f; f.boxmax[i] = 1.0f; }
    return f;
}

int main()
{
    int layouts = 0, tables = 0;
    for (const unsigned long long n : {0ull, 1ull, 2ull, 3ull, 255ull, 256ull, 257ull, 4096ull, 70000ull, 262144ull, 1ull << 30, (1ull << 30) + 1, BRICK_MAX})
        for (const unsigned long long nc : {0ull, 1ull, 300ull, BRICK_MAX}) layouts += check_counts(n, nc);
    // the figures the header and the tests quote; monotone in n; nothing of the frame in it
    CHECK(brick_ray_scratch(0, 0).bytes == 256 && brick_ray_scratch(1, 0).bytes == 512 && brick_ray_scratch(16, 0).bytes == 512 && brick_ray_scratch(17, 0).bytes == 768);
    CHECK(brick_ray_scratch(70000, 0).bytes == 256 + 8 * 262144 && brick_ray_scratch(BRICK_MAX, BRICK_MAX).bytes == 256 + 2 * 8 * (1ull << 32));
    for (unsigned long long n = 0; n < 3000; ++n) CHECK(brick_ray_scratch(n + 1, 0).bytes >= brick_ray_scratch(n, 0).bytes);
    CHECK(brick_check_counts(BRICK_MAX, BRICK_MAX).code == 0 && brick_check_counts(BRICK_MAX + 1, 0).code == KFX_E_RANGE &&
          brick_check_counts(0, BRICK_MAX + 1).code == KFX_E_RANGE && brick_check_counts(~0ull, 0).code == KFX_E_RANGE);
    // the largest table: 2^32 slots, the mask all ones, no shift
    {
        const BrickTable t = brick_table(BRICK_MAX);
        const BrickTableView v = brick_table_view(nullptr, t, BRICK_MAX);
        CHECK(t.cap == (1ull << 32) && v.mask == 0xffffffffu && v.shift == 0 && brick_slot_of(0x12345678u, v.shift) == 0x12345678u * 2654435761u);
    }

    // frames: null, the cell kind, the dimensions kfx_raycast_sdf accepts, the brick limit -- in that order
    BrickGeom g{};
    const kfx_volume ok = frame(40, 24, 16), ragged = frame(44, 29, 35), huge = frame(4096, 4096, 4096);
    CHECK(brick_check_frame(nullptr, g).code == KFX_E_NULL && brick_check_frame(nullptr, KFX_CELL_F32, g).code == KFX_E_NULL);
    CHECK(brick_check_frame(&ok, KFX_CELL_COLOR, g).code == KFX_E_RANGE && brick_check_frame(&ok, -1, g).code == KFX_E_RANGE);
    CHECK(brick_check_frame(&ok, KFX_CELL_F32, g).code == 0 && g.nbx == 5 && g.nby == 3 && g.nbz == 2 && g.nb == 30);
    CHECK(brick_check_frame(&ragged, KFX_CELL_F16, g).code == 0 && g.nbx == 6 && g.nby == 4 && g.nbz == 5 && g.w == 44 && g.h == 29 && g.d == 35);
    CHECK(brick_check_frame(&huge, g).code == 0 && g.nb == 134217728ull);
    for (const size_t bad : {(size_t)0, (size_t)1, (size_t)2, (size_t)65536, ~(size_t)0}) {
        const kfx_volume a = frame(bad, 24, 16), b = frame(40, bad, 16), c = frame(40, 24, bad);
        CHECK(brick_check_frame(&a, g).code == KFX_E_SHAPE && brick_check_frame(&b, KFX_CELL_F32, g).code == KFX_E_SHAPE &&
              brick_check_frame(&c, KFX_CELL_F16, g).code == KFX_E_SHAPE);
        CHECK(brick_check_frame(&a, 7, g).code == KFX_E_RANGE);   // (the kind before the dimensions)
    }
    const kfx_volume edge = frame(3, 3, 3), big = frame(65535, 65535, 65535), most = frame(65535, 65535, 24);
    CHECK(brick_check_frame(&edge, g).code == 0 && g.nb == 1);
    CHECK(brick_check_frame(&big, g).code == KFX_E_RANGE);   // 2^39 bricks
    CHECK(brick_check_frame(&most, g).code == 0 && g.nb == 201326592ull);

    // an id list: nothing asked of an empty one; present, then aligned
    const char* const p = (const char*)((uintptr_t)1 << 20);
    CHECK(brick_ray_check_ids(nullptr, 0).code == 0 && brick_ray_check_ids(p + 1, 0).code == 0);
    CHECK(brick_ray_check_ids(nullptr, 1).code == KFX_E_NULL && brick_ray_check_ids(p + 2, 1).code == KFX_E_ALIGN && brick_ray_check_ids(p + 4, 1).code == 0);

    // ---- the host model of insert and look-up ----
    const unsigned nb = 6 * 4 * 5, last = nb - 1;
    std::vector<unsigned> probe;
    for (unsigned id = 0; id < nb + 40; ++id) probe.push_back(id);
    probe.push_back(0x7fffffffu); probe.push_back(0xfffffffeu); probe.push_back(BRICK_SLOT_EMPTY);
    tables += check_table({}, nb, probe);                          // no bricks: no table, nothing found, nothing read
    tables += check_table({last}, nb, probe);                      // n = 1: the frame's last brick
    tables += check_table({0}, nb, probe);
    tables += check_table({nb}, nb, probe);                        // n = 1, and that id is no brick of the frame: an empty table
    tables += check_table({3, 3, 7, 3, 7}, nb, probe);             // repeated ids
    tables += check_table({7, 119, 3, 0, 64}, nb, probe);          // unsorted
    tables += check_table({5, nb, nb + 1, 0xfffffffeu, last}, nb, probe);   // ids at and beyond the frame's end
    for (const unsigned n : {1u, 255u, 256u, 257u, 1000u}) {
        const BrickTable t = brick_table(n);
        const unsigned big_nb = 0x7fffffffu;   // the largest frame
        // ascending neighbours, as a packed list; then the top of the largest frame, its last brick included
        std::vector<unsigned> run(n), top(n), congruent(n), colliding;
        for (unsigned i = 0; i < n; ++i) { run[i] = i; top[i] = big_nb - n + i; }
        CHECK(top.back() == big_nb - 1);
        tables += check_table(run, n, probe) + check_table(run, big_nb, probe) + check_table(top, big_nb, probe);
        // every id congruent modulo the capacity
        for (unsigned i = 0; i < n; ++i) congruent[i] = 5 + i * (unsigned)t.cap;
        CHECK(congruent.back() < big_nb);
        tables += check_table(congruent, big_nb, {5u + n * (unsigned)t.cap, 4, 6});
        // every id in one slot of the hash: the longest probe sequence the table can have
        const int shift = 32 - t.log2cap;
        const unsigned slot = brick_slot_of(12345u, shift);
        for (unsigned id = 0; colliding.size() < n && id < big_nb; ++id)
            if (brick_slot_of(id, shift) == slot) colliding.push_back(id);
        CHECK(colliding.size() == n);
        std::vector<unsigned> others;
        for (unsigned id = colliding.back() + 1; others.size() < 8; ++id)
            if (brick_slot_of(id, shift) == slot) others.push_back(id);
        tables += check_table(colliding, big_nb, others);
        // ... and the same behind a stretch of other entries that ends at the table's last slot: the probes wrap
        std::vector<unsigned> wrap;
        for (unsigned id = 0; wrap.size() < n && id < big_nb; ++id)
            if (brick_slot_of(id, shift) == (unsigned)t.cap - 1) wrap.push_back(id);
        tables += check_table(wrap, big_nb, others);
    }
    // a table with no empty slot at all (which no plan builds: cap >= 2 n): a look-up of an id that is not there ends after cap probes
    {
        const BrickTable t = brick_table(4);   // 8 slots
        std::vector<unsigned> slots(2 * (size_t)t.cap);
        for (unsigned k = 0; k < t.cap; ++k) { slots[2 * k] = 1000 + k; slots[2 * k + 1] = k; }
        const BrickTableView full = brick_table_view(slots.data(), t, 8);
        CHECK(brick_table_find(full, 7) == -1 && brick_table_find(full, 1003) == 3);
        CHECK(!brick_table_insert(slots.data(), full.mask, full.shift, 7, 0, host_cas));
        // a position at or beyond n is never handed out, whatever the table holds
        const BrickTableView fewer = brick_table_view(slots.data(), t, 3);
        CHECK(brick_table_find(fewer, 1002) == 2 && brick_table_find(fewer, 1003) == -1);
        ++tables;
    }
    printf("raycast_bricks_host_check: ok (%d layouts, %d tables)\n", layouts, tables);
    return 0;
}
