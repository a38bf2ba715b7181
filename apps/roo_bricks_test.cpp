// roo_bricks_test.cpp -- roo::BrickPack / roo::BrickUnpack from C++ (include/kangaroo/VolumeBricks.h over include/kfx_bricks.h) for
// the three cell types, BoundedVolume<SDF_t>, BoundedVolume<SDF_h> and BoundedVolume<float>, against a loop on the host:
//   * a volume of reset cells with some bricks written packs to exactly those bricks, ascending, each cell verbatim and the
//     positions of a partial brick outside the volume the reset cell's bytes;
//   * after a reset, unpacking the list restores every cell.
// Prints "passed" and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// the reset of the cell type: SdfReset for the SDF cells, a host fill for the colour volume
static void Reset(BoundedVolume<SDF_t, TargetDevice, Manage>& v, float fill) { SdfReset(v, fill); }
static void Reset(BoundedVolume<SDF_h, TargetDevice, Manage>& v, float fill) { SdfReset(v, fill); }
static void Reset(BoundedVolume<float, TargetDevice, Manage>& v, float fill)
{
    std::vector<float> h(v.w * v.h * v.d, fill);
    v.MemcpyFromHost(h.data());
}

template<typename T>
static void Run(int w, int h, int d, float fill)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "cell size");
    const size_t n = (size_t)w * h * d;
    const int nbx = (w + 7) / 8, nby = (h + 7) / 8, nbz = (d + 7) / 8, nb = nbx * nby * nbz;
    const float3 lo = make_float3(-1.0f, -1.0f, 2.0f), hi = make_float3(1.0f, 1.0f, 4.0f);
    BoundedVolume<T, TargetDevice, Manage> vol(w, h, d, lo, hi);
    Reset(vol, fill);
    GpuCheckStatus(kfx_stream_synchronize(0));
    std::vector<T> before = ToHost(vol);
    const T fill_cell = before[n / 2];
    // every third brick gets other bits in all of its cells, one more brick in a single cell
    std::vector<int> want_ids;
    for (int id = 0; id < nb; ++id) {
        const bool all = id % 3 == 1, one = id == nb - 1 && !all;
        if (!all && !one) continue;
        want_ids.push_back(id);
        const int bx = id % nbx, by = (id / nbx) % nby, bz = id / (nbx * nby);
        for (int z = bz * 8; z < bz * 8 + 8 && z < d; ++z)
            for (int y = by * 8; y < by * 8 + 8 && y < h; ++y)
                for (int x = bx * 8; x < bx * 8 + 8 && x < w; ++x) {
                    if (one && (x != bx * 8 || y != by * 8 || z != bz * 8)) continue;
                    const size_t i = ((size_t)z * h + y) * w + x;
                    unsigned words[2] = {0x9e3779b9u * (unsigned)(i + 1), 0x85ebca6bu * (unsigned)(i + 7)};
                    words[0] |= 1u;   // (never the reset cell's bits by accident: its low word is even -- NaN, 0.5f and the half NaN alike)
                    memcpy((void*)&before[i], words, sizeof(T));
                }
    }
    vol.MemcpyFromHost(before.data());
    Image<unsigned char, TargetDevice, Manage> scratch(BrickScratchBytes(vol), 1);
    const size_t live = BrickPlan(vol, fill, scratch.ptr, scratch.w);
    CHECK(live == want_ids.size());
    if (live != want_ids.size()) return;
    Image<unsigned, TargetDevice, Manage> ids(live, 1);
    Image<unsigned char, TargetDevice, Manage> cells(live * BrickBytes(vol), 1);
    BrickPack(vol, fill, scratch.ptr, scratch.w, live, ids.ptr, cells.ptr);
    GpuCheckStatus(kfx_stream_synchronize(0));
    std::vector<unsigned> got_ids(live);
    std::vector<T> got_cells(live * 512);
    GpuCheckStatus(kfx_memcpy_2d(got_ids.data(), live * 4, ids.ptr, live * 4, live * 4, 1, 2, 0));
    GpuCheckStatus(kfx_memcpy_2d((void*)got_cells.data(), live * BrickBytes(vol), cells.ptr, live * BrickBytes(vol), live * BrickBytes(vol), 1, 2, 0));
    size_t wrong = 0;
    for (size_t k = 0; k < live; ++k) {
        CHECK(got_ids[k] == (unsigned)want_ids[k]);
        const int id = want_ids[k], bx = id % nbx, by = (id / nbx) % nby, bz = id / (nbx * nby);
        for (int c = 0; c < 512; ++c) {
            const int x = bx * 8 + (c & 7), y = by * 8 + ((c >> 3) & 7), z = bz * 8 + (c >> 6);
            const bool in = x < w && y < h && z < d;
            const T& expect = in ? before[((size_t)z * h + y) * w + x] : fill_cell;
            wrong += memcmp((const void*)&got_cells[k * 512 + c], (const void*)&expect, sizeof(T)) != 0 ? 1 : 0;
        }
    }
    if (wrong) fprintf(stderr, "cell size %zu: %zu packed cells differ\n", sizeof(T), wrong);
    CHECK(wrong == 0);
    Reset(vol, fill);
    BrickUnpack(vol, ids.ptr, cells.ptr, live);
    GpuCheckStatus(kfx_stream_synchronize(0));
    const std::vector<T> after = ToHost(vol);
    CHECK(memcmp((const void*)after.data(), (const void*)before.data(), n * sizeof(T)) == 0);
}

int main()
{
    Run<SDF_t>(40, 24, 16, NAN);
    Run<SDF_h>(70, 13, 24, NAN);
    Run<float>(37, 24, 12, 0.5f);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("passed\n");
    return 0;
}
