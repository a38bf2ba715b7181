// brick_pool_host_check.cpp -- the host side of the brick pool (kangaroo_amd/csrc/brick_pool_host.h) under the host sanitizers, on a
// machine without a device: the carving of a pool and of its scratch -- every part inside the total, aligned, none overlapping, the
// sums the public header states -- the refusals of the kind, the pool, the scratch and a key range, each with its code and in its
// order, and a host model of the pool: keys, free stack and counters on host arrays of exactly the pool's sizes, updated through the
// functions the kernels call (brick_pool_key_in_box, brick_pool_key_of, brick_pool_spill_index, brick_pool_push_index,
// brick_pool_after_spill, brick_pool_after_take), so an index that left the pool would be an out-of-bounds access the address sanitizer
// reports.  A few thousand random spill, restore and discard steps run against a std::map: negative keys, keys at both ends of
// int32, boxes that overlap what the pool holds (re-spilled keys), more live bricks than free slots (overflow).  After every step the
// occupied slots and the free stack partition [0, capacity), the map matches, and the slots taken are the ones the rule names.
// The kernels are not covered here (tests/test_gpu_brick_pool.py), nor the entry points (tests/test_abi_brick_pool_cpu.py).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/brick_pool_host_check.cpp -o check && ./check
#include <algorithm>
#include <array>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../kangaroo_amd/csrc/brick_pool_host.h"

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
    } while (0)

using namespace kfx;

static size_t r256(unsigned long long n) { return (size_t)((n + 255) / 256 * 256); }

static void check_layouts()
{
    for (const unsigned long long cap : {1ull, 2ull, 15ull, 16ull, 17ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 65537ull, 262144ull, 0x7fffffffull})
        for (const size_t cb : {(size_t)4, (size_t)8}) {
            const BrickPoolLayout p = brick_pool_layout(cb, cap);
            CHECK(p.bytes == 256 + r256(16 * cap) + r256(4 * cap) + 512 * cb * cap);   // include/kfx_brick_pool.h
            CHECK(p.hdr == 0 && p.keys == 256 && sizeof(BrickPoolHeader) <= 256 && sizeof(BrickPoolKey) == 16);
            CHECK(p.keys + 16 * cap <= p.free && p.free + 4 * cap <= p.cells && p.cells + p.brick_bytes * cap <= p.bytes);
            CHECK(p.keys % 256 == 0 && p.free % 256 == 0 && p.cells % 256 == 0 && p.bytes % 256 == 0 && p.brick_bytes == 512 * cb);
            for (const unsigned long long nb : {0ull, 1ull, 255ull, 256ull, 257ull, 70000ull, 0x7fffffffull}) {
                const BrickPoolScratch s = brick_pool_scratch(nb, cap);
                const unsigned long long n = std::max(nb, cap), nblk = (n + 255) / 256;
                CHECK(s.n == n && s.nblk == nblk);
                CHECK(s.bytes == 256 + r256(n) + 2 * r256(4 * nblk) + r256(4 * n));
                CHECK(s.hdr == 0 && s.flags == 256 && s.flags + n <= s.part && s.part + 4 * nblk <= s.base && s.base + 4 * nblk <= s.list && s.list + 4 * n <= s.bytes);
                CHECK(s.part % 256 == 0 && s.base % 256 == 0 && s.list % 256 == 0);
                CHECK(brick_pool_scratch(0, cap).bytes <= s.bytes);   // the scratch of a view serves a discard
            }
        }
}

static void check_refusals()
{
    size_t cb = 0;
    CHECK(brick_pool_check_kind(KFX_CELL_F32, 1, cb).code == 0 && cb == 8);
    CHECK(brick_pool_check_kind(KFX_CELL_F16, 1, cb).code == 0 && cb == 4);
    CHECK(brick_pool_check_kind(KFX_CELL_COLOR, 0x7fffffffull, cb).code == 0 && cb == 4);
    CHECK(brick_pool_check_kind(3, 1, cb).code == KFX_E_RANGE && brick_pool_check_kind(-1, 0, cb).code == KFX_E_RANGE);
    CHECK(brick_pool_check_kind(KFX_CELL_F32, 0, cb).code == KFX_E_RANGE && brick_pool_check_kind(KFX_CELL_F32, 0x80000000ull, cb).code == KFX_E_RANGE);
    void* const good = (void*)(uintptr_t)(1 << 20);
    void* const odd = (void*)(uintptr_t)((1 << 20) + 128);
    const size_t need = brick_pool_layout(8, 100).bytes, sneed = brick_pool_scratch(300, 100).bytes;
    CHECK(brick_pool_check_pool(good, need, 8, 100).code == 0);
    CHECK(brick_pool_check_pool(nullptr, 0, 8, 100).code == KFX_E_NULL);           // null before size before alignment
    CHECK(brick_pool_check_pool(odd, need - 1, 8, 100).code == KFX_E_SHAPE);
    CHECK(brick_pool_check_pool(odd, need, 8, 100).code == KFX_E_ALIGN);
    CHECK(brick_pool_check_scratch(300, 100, good, sneed).code == 0);
    CHECK(brick_pool_check_scratch(300, 100, nullptr, 0).code == KFX_E_NULL);
    CHECK(brick_pool_check_scratch(300, 100, odd, sneed - 1).code == KFX_E_SHAPE);
    CHECK(brick_pool_check_scratch(300, 100, odd, sneed).code == KFX_E_ALIGN);
    const int nb[3] = {4, 3, 2};
    const int lo[3] = {INT_MIN, INT_MIN, INT_MIN}, hi[3] = {INT_MAX - 3, INT_MAX - 2, INT_MAX - 1}, over[3] = {0, INT_MAX - 1, 0};
    CHECK(brick_pool_check_keys(lo, nb).code == 0 && brick_pool_check_keys(hi, nb).code == 0 && brick_pool_check_keys(over, nb).code == KFX_E_RANGE);
}

typedef std::array<int, 3> Key;

// the pool on the host: what the kernels do, step by step, through the shared functions
struct Model {
    unsigned long long capacity;
    BrickPoolHeader h;
    std::vector<BrickPoolKey> keys;
    std::vector<unsigned> free;
    std::vector<unsigned long long> cells;   // one word stands for a slot's payload

    explicit Model(unsigned long long cap) : capacity(cap), keys(cap), free(cap), cells(cap, 0)
    {
        for (unsigned long long i = 0; i < cap; ++i) {    // k_pool_init
            keys[i] = BrickPoolKey{0, 0, 0, BRICK_POOL_FREE};
            free[i] = (unsigned)(cap - 1 - i);
        }
        h = BrickPoolHeader{cap, 0, 0, 0, 0, (unsigned)cap};
    }
    // k_pool_match + scan + k_pool_take + k_pool_header; the slots taken, ascending
    std::vector<unsigned> take(const BrickPoolBox& box, bool restore)
    {
        std::vector<unsigned> list;
        const unsigned long long free_n = brick_pool_free_n(h.free_n, capacity);
        for (unsigned slot = 0; slot < capacity; ++slot) {
            unsigned id;
            if (keys[slot].state != BRICK_POOL_OCCUPIED || !brick_pool_key_in_box(box, keys[slot].bx, keys[slot].by, keys[slot].bz, &id)) continue;
            const long long at = brick_pool_push_index(free_n, list.size(), capacity);
            CHECK(at >= 0);
            free.at((size_t)at) = slot;
            keys[slot].state = BRICK_POOL_FREE;
            list.push_back(slot);
        }
        brick_pool_after_take(h, list.size(), capacity, restore);
        return list;
    }
    // the discard, then k_pool_put over the live ids (ascending) + k_pool_header; the slots written, by rank
    std::vector<unsigned> spill(const BrickPoolBox& box, const std::vector<unsigned>& live, unsigned long long payload)
    {
        take(box, false);
        std::vector<unsigned> slots;
        const unsigned long long free_n = brick_pool_free_n(h.free_n, capacity);
        for (size_t r = 0; r < live.size(); ++r) {
            const long long at = brick_pool_spill_index(free_n, r);
            if (at < 0) continue;
            const unsigned slot = free.at((size_t)at);
            CHECK(brick_pool_slot_ok(slot, capacity));
            keys[slot] = brick_pool_key_of(box, live[r]);
            cells[slot] = payload + live[r];
            slots.push_back(slot);
        }
        brick_pool_after_spill(h, live.size(), capacity);
        return slots;
    }
};

static bool in_box(const BrickPoolBox& b, const Key& k)
{
    for (int a = 0; a < 3; ++a)
        if ((long long)k[a] < b.key0[a] || (long long)k[a] > (long long)b.key0[a] + b.nb[a] - 1) return false;
    return true;
}

static void check_model(unsigned long long capacity, unsigned seed, int steps)
{
    std::mt19937 rng(seed);
    Model m(capacity);
    std::map<Key, unsigned long long> ref;
    unsigned long long spilled = 0, restored = 0, dropped = 0;
    // boxes live near one of three corners of key space: around zero (negative keys), at the bottom and at the top of int32
    const int corner[3] = {-4, INT_MIN, INT_MAX - 11};
    for (int step = 0; step < steps; ++step) {
        BrickPoolBox box;
        const int c = corner[rng() % 3];
        for (int a = 0; a < 3; ++a) {
            box.nb[a] = 1 + (int)(rng() % 5);
            box.key0[a] = c + (int)(rng() % (unsigned)(12 - box.nb[a] + 1));
        }
        CHECK(brick_pool_check_keys(box.key0, box.nb).code == 0);
        const unsigned nb = (unsigned)(box.nb[0] * box.nb[1] * box.nb[2]);
        const unsigned op = rng() % 8;
        const std::vector<unsigned> free_before = m.free;
        if (op < 4) {                                   // spill
            std::vector<unsigned> live;
            const unsigned density = 1 + rng() % 4;
            for (unsigned id = 0; id < nb; ++id)
                if (rng() % 4 < density) live.push_back(id);
            const unsigned long long payload = ((unsigned long long)(step + 1)) << 32;
            for (auto it = ref.begin(); it != ref.end();) it = in_box(box, it->first) ? ref.erase(it) : std::next(it);
            const unsigned long long free_n = capacity - ref.size();
            const std::vector<unsigned> slots = m.spill(box, live, payload);
            // the rule: the r-th live brick took the slot free[free_n - 1 - r] of the stack as the discard left it
            CHECK(slots.size() == std::min<unsigned long long>(live.size(), free_n));
            for (size_t r = 0; r < live.size(); ++r) {
                const unsigned id = live[r];
                const Key k = {box.key0[0] + (int)(id % (unsigned)box.nb[0]), box.key0[1] + (int)(id / (unsigned)box.nb[0] % (unsigned)box.nb[1]),
                               box.key0[2] + (int)(id / (unsigned)(box.nb[0] * box.nb[1]))};
                if (r < free_n) {
                    CHECK(slots[r] == m.free[(size_t)(free_n - 1 - r)]);   // (a spill pops: the entries stay where they were)
                    ref[k] = payload + id;
                    ++spilled;
                } else {
                    ++dropped;
                }
            }
        } else {                                        // restore / discard
            const bool restore = op < 6;
            std::vector<Key> gone;
            for (auto it = ref.begin(); it != ref.end();)
                if (in_box(box, it->first)) { gone.push_back(it->first); it = ref.erase(it); } else ++it;
            const unsigned long long free_n = capacity - ref.size() - gone.size();
            const std::vector<unsigned> list = m.take(box, restore);
            CHECK(list.size() == gone.size() && std::is_sorted(list.begin(), list.end()));
            for (size_t i = 0; i < list.size(); ++i) {
                CHECK(m.free[(size_t)(free_n + i)] == list[i]);           // pushed in ascending slot order
                const BrickPoolKey& k = m.keys[list[i]];
                CHECK(std::find(gone.begin(), gone.end(), Key{k.bx, k.by, k.bz}) != gone.end());
            }
            for (size_t i = 0; i < (size_t)free_n; ++i) CHECK(m.free[i] == free_before[i]);
            if (restore) restored += gone.size();
        }
        // occupied slots and the free stack partition [0, capacity); the map matches; the counters
        CHECK(m.h.free_n == capacity - ref.size() && m.h.spilled == spilled && m.h.restored == restored && m.h.dropped == dropped);
        std::vector<int> seen(capacity, 0);
        for (unsigned long long i = 0; i < m.h.free_n; ++i) {
            CHECK(m.free[i] < capacity && m.keys[m.free[i]].state == BRICK_POOL_FREE);
            ++seen[m.free[i]];
        }
        size_t occupied = 0;
        for (unsigned slot = 0; slot < capacity; ++slot) {
            if (m.keys[slot].state != BRICK_POOL_OCCUPIED) continue;
            ++seen[slot];
            ++occupied;
            const auto it = ref.find(Key{m.keys[slot].bx, m.keys[slot].by, m.keys[slot].bz});
            CHECK(it != ref.end() && it->second == m.cells[slot]);
        }
        CHECK(occupied == ref.size());
        for (unsigned slot = 0; slot < capacity; ++slot) CHECK(seen[slot] == 1);
    }
    CHECK(spilled > 0 && dropped > 0 && (restored > 0 || capacity == 1));   // (one slot: a box seldom meets the one key)
}

// a header and keys that hold anything: every index the rules give stays inside the pool
static void check_overwritten()
{
    const unsigned long long cap = 10;
    for (const unsigned long long free_n : {0ull, 3ull, 10ull, 11ull, ~0ull}) {
        const unsigned long long f = brick_pool_free_n(free_n, cap);
        CHECK(f <= cap);
        for (unsigned long long r = 0; r < 2 * cap; ++r) {
            const long long a = brick_pool_spill_index(f, r), b = brick_pool_push_index(f, r, cap);
            CHECK(a < (long long)cap && b < (long long)cap && (a >= 0) == (r < f));
        }
        BrickPoolHeader h{free_n, 1, 2, 3, 0, (unsigned)cap};
        brick_pool_after_take(h, 7, cap, true);
        CHECK(h.free_n <= cap);
        brick_pool_after_spill(h, 1000, cap);
        CHECK(h.free_n == 0);
    }
    const BrickPoolBox box{{INT_MAX - 2, -1, INT_MIN}, {3, 2, 4}};
    unsigned id = 0;
    for (const int v : {INT_MIN, -2, -1, 0, 1, INT_MAX - 3, INT_MAX - 2, INT_MAX})
        for (const int w : {INT_MIN, INT_MIN + 3, INT_MIN + 4, -1, 0, 1, INT_MAX})
            if (brick_pool_key_in_box(box, v, w == INT_MIN ? -1 : 0, w, &id)) {
                CHECK(id < 24);
                const BrickPoolKey k = brick_pool_key_of(box, id);
                CHECK(k.bx == v && k.bz == w && k.state == BRICK_POOL_OCCUPIED);
            }
    CHECK(!brick_pool_slot_ok(10, cap) && brick_pool_slot_ok(9, cap) && !brick_pool_slot_ok(0xffffffffu, cap));
}

int main()
{
    check_layouts();
    check_refusals();
    check_model(1, 1, 300);
    check_model(7, 2, 1500);       // smaller than most boxes: overflow at nearly every spill
    check_model(64, 3, 1500);
    check_model(300, 4, 1500);     // larger than what the boxes can hold together at one corner
    check_overwritten();
    printf("brick_pool_host_check: ok\n");
    return 0;
}
