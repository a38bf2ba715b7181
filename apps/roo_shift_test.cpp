// roo_shift_test.cpp -- roo::VolumeShift from C++ (include/kangaroo/VolumeShift.h over include/kfx_shift.h) for the three cell
// types, BoundedVolume<SDF_t>, BoundedVolume<SDF_h> and BoundedVolume<float>, against a loop on the host:
//   * every cell of the shifted volume holds the bytes of its source cell, or -- where the source lies outside -- the bytes
//     SdfReset(vol, fill) writes (colour: fill itself), for shifts that take the direct path, the staged path and the single fill;
//   * vol.bbox is VoxelPositionInUnits of the shifted first and last voxel, bit for bit.
// Prints "passed" and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <kangaroo/kangaroo.h>
#include <kangaroo/VolumeShift.h>

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

static bool SameBits(float3 a, float3 b) { return memcmp(&a, &b, sizeof(a)) == 0; }

// the reset of the cell type: SdfReset for the SDF cells, Fill for the colour volume
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
    const int shifts[][3] = {{3, -2, 5}, {-7, 5, -1}, {8, 0, 0}, {0, -3, 0}, {-1, 0, 0}, {0, 0, 7}, {w, 0, 0}, {0, 0, -d}};
    const size_t n = (size_t)w * h * d;
    const float3 lo = make_float3(-1.0f, -1.0f, 2.0f), hi = make_float3(1.0f, 1.0f, 4.0f);
    // the bytes of a reset cell
    BoundedVolume<T, TargetDevice, Manage> blank(w, h, d, lo, hi);
    Reset(blank, fill);
    GpuCheckStatus(kfx_stream_synchronize(0));
    const T fill_cell = ToHost(blank)[n / 2];
    for (const auto& s : shifts) {
        BoundedVolume<T, TargetDevice, Manage> vol(w, h, d, lo, hi);
        std::vector<T> before(n);
        std::vector<unsigned> words(n * sizeof(T) / 4);
        for (size_t i = 0; i < words.size(); ++i) words[i] = 0x9e3779b9u * (unsigned)(i + 1);   // any bits, NaN patterns among them
        memcpy((void*)before.data(), words.data(), n * sizeof(T));
        vol.MemcpyFromHost(before.data());
        const float3 want_lo = vol.VoxelPositionInUnits(s[0], s[1], s[2]);
        const float3 want_hi = vol.VoxelPositionInUnits(w - 1 + s[0], h - 1 + s[1], d - 1 + s[2]);
        const size_t bytes = VolumeShiftScratchBytes(vol, s[0], s[1], s[2], 3);
        CHECK((bytes != 0) == (s[2] == 0 && abs(s[0]) < w && abs(s[1]) < h));
        Image<unsigned char, TargetDevice, Manage> scratch(bytes ? bytes : 256, 1);
        VolumeShift(vol, s[0], s[1], s[2], fill, bytes ? (void*)scratch.ptr : nullptr, bytes);
        GpuCheckStatus(kfx_stream_synchronize(0));
        CHECK(SameBits(vol.bbox.Min(), want_lo) && SameBits(vol.bbox.Max(), want_hi));
        const std::vector<T> after = ToHost(vol);
        size_t wrong = 0, kept = 0;
        for (int z = 0; z < d; ++z)
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    const int xs = x + s[0], ys = y + s[1], zs = z + s[2];
                    const bool in = xs >= 0 && xs < w && ys >= 0 && ys < h && zs >= 0 && zs < d;
                    const T& expect = in ? before[((size_t)zs * h + ys) * w + xs] : fill_cell;
                    kept += in ? 1 : 0;
                    wrong += memcmp((const void*)&after[((size_t)z * h + y) * w + x], (const void*)&expect, sizeof(T)) != 0 ? 1 : 0;
                }
        if (wrong) fprintf(stderr, "cell size %zu, shift (%d, %d, %d): %zu cells differ\n", sizeof(T), s[0], s[1], s[2], wrong);
        CHECK(wrong == 0);
        CHECK((kept == 0) == (abs(s[0]) >= w || abs(s[1]) >= h || abs(s[2]) >= d));
    }
}

int main()
{
    Run<SDF_t>(40, 24, 16, NAN);
    Run<SDF_h>(72, 16, 24, NAN);
    Run<float>(40, 24, 16, 0.5f);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("passed\n");
    return 0;
}
