// roo_brick_pool_test.cpp -- the brick pool from C++ (roo::BrickPool* of include/kangaroo/VolumeBricks.h over include/kfx_brick_pool.h)
// for the three cell types, BoundedVolume<SDF_t>, BoundedVolume<SDF_h> and BoundedVolume<float>, against a loop on the host:
//   * a sub-view of a volume of reset cells with some bricks written spills into a pool; the pool's bytes, read through the documented
//     layout as a map key -> 512 cells, are exactly the live bricks of the view under key0 + (bx, by, bz), slot r holding the r-th of
//     them, the positions of a partial brick outside the view the reset cell's bytes, and the counters say so;
//   * the whole volume overwritten, a restore puts back the cells of those bricks inside the view and nothing else: every cell of the
//     storage is compared; the pool is empty afterwards.
// Prints "passed" and exits 0 when every check holds.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include <kangaroo/kangaroo.h>
#include <kangaroo/VolumeBricks.h>

using namespace roo;

static int g_fail = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { ++g_fail; fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

template<typename T>
static std::vector<T> ToHost(const BoundedVolume<T, TargetDevice, Manage>& v)
{
    std::vector<T> out(v.w * v.h * v.d);
    const size_t row = v.w * sizeof(T);
    GpuCheckStatus(kfx_memcpy_2d(out.data(), row, v.ptr, v.pitch, row, v.h * v.d, 2, 0));
    return out;
}

static void Reset(BoundedVolume<SDF_t, TargetDevice, Manage>& v, float fill) { SdfReset(v, fill); }
static void Reset(BoundedVolume<SDF_h, TargetDevice, Manage>& v, float fill) { SdfReset(v, fill); }
static void Reset(BoundedVolume<float, TargetDevice, Manage>& v, float fill)
{
    std::vector<float> h(v.w * v.h * v.d, fill);
    v.MemcpyFromHost(h.data());
}

static size_t Round256(size_t n) { return (n + 255) / 256 * 256; }

typedef std::array<int, 3> Key;
typedef std::vector<unsigned char> Bytes;

template<typename T>
static void Run(int w, int h, int d, int x0, int y0, int z0, int vw, int vh, int vd, float fill)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "cell size");
    const size_t n = (size_t)w * h * d, capacity = 64, brick = 512 * sizeof(T);
    const int nbx = (vw + 7) / 8, nby = (vh + 7) / 8, nbz = (vd + 7) / 8, nb = nbx * nby * nbz;
    const int key0[3] = {-3, 5, 1000};
    const float3 lo = make_float3(-1.0f, -1.0f, 2.0f), hi = make_float3(1.0f, 1.0f, 4.0f);
    BoundedVolume<T, TargetDevice, Manage> vol(w, h, d, lo, hi);
    Reset(vol, fill);
    GpuCheckStatus(kfx_stream_synchronize(0));
    std::vector<T> before = ToHost(vol);
    const T fill_cell = before[n / 2];
    const auto at = [&](int x, int y, int z) { return ((size_t)(z0 + z) * h + (y0 + y)) * w + (x0 + x); };   // a cell of the view
    // every third brick of the view gets other bits in all of its cells inside the view, the last brick in a single cell; the cells
    // around the view get other bits too: they are no business of the pool
    for (size_t i = 0; i < n; ++i) {
        const int x = (int)(i % w) - x0, y = (int)(i / w % h) - y0, z = (int)(i / ((size_t)w * h)) - z0;
        if (x >= 0 && y >= 0 && z >= 0 && x < vw && y < vh && z < vd) continue;
        const unsigned words[2] = {0x7f4a7c15u * (unsigned)(i + 3) | 1u, 0x2545f491u * (unsigned)(i + 5)};
        memcpy((void*)&before[i], words, sizeof(T));
    }
    std::vector<int> want_ids;
    for (int id = 0; id < nb; ++id) {
        const bool all = id % 3 == 1, one = id == nb - 1 && !all;
        if (!all && !one) continue;
        want_ids.push_back(id);
        const int bx = id % nbx, by = (id / nbx) % nby, bz = id / (nbx * nby);
        for (int z = bz * 8; z < bz * 8 + 8 && z < vd; ++z)
            for (int y = by * 8; y < by * 8 + 8 && y < vh; ++y)
                for (int x = bx * 8; x < bx * 8 + 8 && x < vw; ++x) {
                    if (one && (x != bx * 8 || y != by * 8 || z != bz * 8)) continue;
                    const size_t i = at(x, y, z);
                    unsigned words[2] = {0x9e3779b9u * (unsigned)(i + 1), 0x85ebca6bu * (unsigned)(i + 7)};
                    words[0] |= 1u;   // (never the reset cell's bits by accident: its low word is even -- NaN, 0.5f and the half NaN alike)
                    memcpy((void*)&before[i], words, sizeof(T));
                }
    }
    vol.MemcpyFromHost(before.data());
    BoundedVolume<T, TargetDevice, DontManage> view(vol.SubVolume(make_int3(x0, y0, z0), make_int3(vw, vh, vd)), vol.bbox);

    const size_t pool_bytes = BrickPoolBytes<T>(capacity), scratch_bytes = BrickPoolScratchBytes(view, capacity);
    CHECK(pool_bytes == 256 + Round256(16 * capacity) + Round256(4 * capacity) + brick * capacity && scratch_bytes > 0);
    Image<unsigned char, TargetDevice, Manage> pool(pool_bytes, 1), scratch(scratch_bytes, 1);
    BrickPoolInit<T>(pool.ptr, pool_bytes, capacity);
    BrickPoolSpill(pool.ptr, pool_bytes, capacity, view, fill, key0, scratch.ptr, scratch_bytes);
    unsigned long long st[4] = {9, 9, 9, 9};
    BrickPoolStats<T>(pool.ptr, pool_bytes, capacity, st);
    CHECK(st[0] == want_ids.size() && st[1] == want_ids.size() && st[2] == 0 && st[3] == 0);

    // the pool as a map, through the documented layout
    Bytes host(pool_bytes);
    GpuCheckStatus(kfx_memcpy_2d(host.data(), pool_bytes, pool.ptr, pool_bytes, pool_bytes, 1, 2, 0));
    const int* keys = (const int*)(host.data() + 256);
    const unsigned char* cells = host.data() + 256 + Round256(16 * capacity) + Round256(4 * capacity);
    std::map<Key, Bytes> got, want;
    for (size_t s = 0; s < capacity; ++s)
        if (keys[4 * s + 3] == 1) got[Key{keys[4 * s], keys[4 * s + 1], keys[4 * s + 2]}] = Bytes(cells + s * brick, cells + (s + 1) * brick);
    for (size_t r = 0; r < want_ids.size(); ++r) {
        const int id = want_ids[r], bx = id % nbx, by = (id / nbx) % nby, bz = id / (nbx * nby);
        Bytes b(brick);
        for (int c = 0; c < 512; ++c) {
            const int x = bx * 8 + (c & 7), y = by * 8 + ((c >> 3) & 7), z = bz * 8 + (c >> 6);
            const T& cell = x < vw && y < vh && z < vd ? before[at(x, y, z)] : fill_cell;
            memcpy(b.data() + (size_t)c * sizeof(T), (const void*)&cell, sizeof(T));
        }
        want[Key{key0[0] + bx, key0[1] + by, key0[2] + bz}] = b;
        CHECK(keys[4 * r + 3] == 1 && keys[4 * r] == key0[0] + bx && keys[4 * r + 1] == key0[1] + by && keys[4 * r + 2] == key0[2] + bz);   // slot r: the r-th id
    }
    CHECK(got.size() == want.size());
    CHECK(got == want);

    // the slots, gathered on the device in reverse order, are the same bytes
    {
        const size_t m = want_ids.size();
        std::vector<unsigned> slots(m);
        for (size_t i = 0; i < m; ++i) slots[i] = (unsigned)(m - 1 - i);
        Image<unsigned, TargetDevice, Manage> dslots(m, 1);
        Image<unsigned char, TargetDevice, Manage> dcells(m * brick, 1);
        GpuCheckStatus(kfx_memcpy_2d(dslots.ptr, m * 4, slots.data(), m * 4, m * 4, 1, 1, 0));
        BrickPoolGather<T>(pool.ptr, pool_bytes, capacity, dslots.ptr, m, dcells.ptr);
        GpuCheckStatus(kfx_stream_synchronize(0));
        Bytes g(m * brick);
        GpuCheckStatus(kfx_memcpy_2d(g.data(), m * brick, dcells.ptr, m * brick, m * brick, 1, 2, 0));
        for (size_t i = 0; i < m; ++i) CHECK(memcmp(g.data() + i * brick, cells + (m - 1 - i) * brick, brick) == 0);
    }

    // every cell of the volume overwritten; the restore writes the cells of the spilled bricks inside the view, and nothing else
    std::vector<T> junk(n);
    for (size_t i = 0; i < n; ++i) {
        const unsigned words[2] = {0xc2b2ae35u * (unsigned)(i + 11), 0x27d4eb2fu * (unsigned)(i + 13)};
        memcpy((void*)&junk[i], words, sizeof(T));
    }
    vol.MemcpyFromHost(junk.data());
    BrickPoolRestore(pool.ptr, pool_bytes, capacity, view, key0, scratch.ptr, scratch_bytes);
    GpuCheckStatus(kfx_stream_synchronize(0));
    std::vector<T> expect = junk;
    for (const int id : want_ids) {
        const int bx = id % nbx, by = (id / nbx) % nby, bz = id / (nbx * nby);
        for (int z = bz * 8; z < bz * 8 + 8 && z < vd; ++z)
            for (int y = by * 8; y < by * 8 + 8 && y < vh; ++y)
                for (int x = bx * 8; x < bx * 8 + 8 && x < vw; ++x) memcpy((void*)&expect[at(x, y, z)], (const void*)&before[at(x, y, z)], sizeof(T));
    }
    const std::vector<T> after = ToHost(vol);
    CHECK(memcmp((const void*)after.data(), (const void*)expect.data(), n * sizeof(T)) == 0);
    BrickPoolStats<T>(pool.ptr, pool_bytes, capacity, st);
    CHECK(st[0] == 0 && st[1] == want_ids.size() && st[2] == want_ids.size() && st[3] == 0);
}

int main()
{
    Run<SDF_t>(40, 24, 16, 3, 2, 1, 32, 16, 12, NAN);
    Run<SDF_h>(72, 16, 24, 1, 2, 1, 66, 9, 20, NAN);
    Run<float>(37, 24, 12, 0, 3, 2, 37, 20, 9, 0.5f);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("passed\n");
    return 0;
}
