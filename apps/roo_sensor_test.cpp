// roo_sensor_test.cpp -- roo::DepthInput and roo::BilateralFilterDepth from C++ (include/kangaroo/DepthInput.h over
// include/kfx_sensor.h) against the separate calls ElementwiseScaleBias<float, unsigned short, float> + BilateralFilter<float, float>:
//   * a stream of 16-bit millimetre frames through a two-slot ring, each submitted one frame ahead of its Filter: the filtered
//     image and the metres image of every frame equal the separate calls' bit for bit, in both numerics modes;
//   * the ring refuses a third image while two are pending and takes it after one Filter.
// Prints "passed" and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <kangaroo/kangaroo.h>
#include <kangaroo/DepthInput.h>

using namespace roo;

static int g_fail = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { ++g_fail; fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// a tilted wall between 1.5 m and 2.9 m in millimetres, a block of invalid readings, one saturated pixel; frame k is k mm further
static void MakeFrame(std::vector<unsigned short>& mm, int w, int h, int k)
{
    mm.resize((size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            unsigned v = 1500u + (unsigned)(x * 11 + y * 7) + 40u * (unsigned)((x / 9 + y / 5) & 1) + (unsigned)k;
            if (x >= 20 && x < 31 && y >= 12 && y < 19) v = 0;
            mm[(size_t)y * w + x] = (unsigned short)v;
        }
    mm[(size_t)(h - 3) * w + 5] = 65535;
}

static bool SameBits(const std::vector<float>& a, const std::vector<float>& b)
{
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

static std::vector<float> ToHost(const Image<float>& im)
{
    std::vector<float> out((size_t)im.w * im.h);
    im.MemcpyToHost(out.data());
    return out;
}

int main()
{
    const int w = 83, h = 61, frames = 5;
    const float s = 1.0f / 1000.0f, gs = 1.5f, gr = 0.1f, minval = 0.2f;
    const uint size = 3;
    for (int mode = KFX_MATH_EXACT; mode <= KFX_MATH_FAST; ++mode) {
        kfx_set_math_mode(mode);
        Image<unsigned short, TargetDevice, Manage> dRaw(w, h);
        Image<float, TargetDevice, Manage> dMeters(w, h), dFiltered(w, h), rMeters(w, h), rFiltered(w, h), oMeters(w, h), oFiltered(w, h);
        DepthInput<unsigned short> input(w, h, s);
        std::vector<unsigned short> mm;
        const auto submit = [&](int k) {
            Image<unsigned short, TargetHost, DontManage> buf = input.Acquire();
            CHECK(buf.ptr != 0 && buf.w == (size_t)w && buf.h == (size_t)h);
            if (!buf.ptr) return;
            MakeFrame(mm, w, h, k);
            for (int y = 0; y < h; ++y) memcpy((unsigned char*)buf.ptr + (size_t)y * buf.pitch, &mm[(size_t)y * w], (size_t)w * 2);
            input.Submit();
        };
        submit(0);
        for (int k = 0; k < frames; ++k) {
            if (k + 1 < frames) submit(k + 1);
            CHECK(input.Pending() == (k + 1 < frames ? 2 : 1));
            if (k == 1) {   // two pending: the ring is full, and says so without changing anything
                CHECK(input.Acquire().ptr == 0);
                CHECK(input.Pending() == 2);
            }
            input.Filter(dFiltered, dMeters, gs, gr, size, minval);
            CHECK(input.Pending() == (k + 1 < frames ? 1 : 0));
            // the separate calls on the same frame
            MakeFrame(mm, w, h, k);
            dRaw.MemcpyFromHost(mm.data());
            ElementwiseScaleBias<float, unsigned short, float>(rMeters, dRaw, s, 0.f);
            BilateralFilter<float, float>(rFiltered, rMeters, gs, gr, size, minval);
            // ... and the stateless operator
            BilateralFilterDepth<unsigned short>(oFiltered, oMeters, dRaw, s, 0.f, gs, gr, size, minval);
            GpuCheckStatus(kfx_stream_synchronize(0));
            const std::vector<float> rf = ToHost(rFiltered), rm = ToHost(rMeters);
            CHECK(SameBits(ToHost(dFiltered), rf));
            CHECK(SameBits(ToHost(dMeters), rm));
            CHECK(SameBits(ToHost(oFiltered), rf));
            CHECK(SameBits(ToHost(oMeters), rm));
            size_t finite = 0;
            for (float v : rf) finite += std::isfinite(v) ? 1 : 0;
            CHECK(finite > rf.size() / 2 && finite < rf.size());
        }
        CHECK(input.Pending() == 0);
    }
    kfx_set_math_mode(KFX_MATH_EXACT);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("passed\n");
    return 0;
}
