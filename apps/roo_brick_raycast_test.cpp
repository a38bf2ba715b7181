// roo_brick_raycast_test.cpp -- roo::RaycastBricksPlan / RaycastSdfBricks from C++ (include/kangaroo/VolumeBricks.h over
// include/kfx_raycast_bricks.h): a small volume with a sphere and some unobserved cells is packed into bricks, the bricks are rendered,
// the volume is rendered (roo::RaycastSdf), and the images are compared bit for bit:
//   * with every brick listed;
//   * with a fifth of the bricks left out (brick (bx, by, bz) where (bx + 2 by + 3 bz) % 5 == 0), against the volume reset and the
//     others unpacked -- one plan, two poses;
//   * the colour overload without colour bricks: img is 0.5 at every hit, depth and normals as before.
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

static const int W = 67, H = 45;   // a ragged image
// the comparator must hit on at least 15 % of the pixels and miss on at least 15 %: a comparison of empty images shows nothing
static const size_t FLOOR = (size_t)(0.15 * W * H) + 1;

struct Views {
    std::vector<float> d, i;
    std::vector<float4> n;
    size_t hits() const
    {
        size_t k = 0;
        for (const float v : d) k += v > 0;
        return k;
    }
};

struct Targets {
    Image<float, TargetDevice, Manage> depth, img;
    Image<float4, TargetDevice, Manage> norm;
    Targets() : depth(W, H), img(W, H), norm(W, H) {}
    Views Read()
    {
        Views v;
        v.d.resize((size_t)W * H); v.i.resize((size_t)W * H); v.n.resize((size_t)W * H);
        depth.MemcpyToHost(v.d.data()); img.MemcpyToHost(v.i.data()); norm.MemcpyToHost(v.n.data());
        return v;
    }
};

static bool SameBits(const Views& a, const Views& b, bool with_img = true)
{
    return memcmp(a.d.data(), b.d.data(), a.d.size() * 4) == 0 && memcmp(a.n.data(), b.n.data(), a.n.size() * 16) == 0 &&
           (!with_img || memcmp(a.i.data(), b.i.data(), a.i.size() * 4) == 0);
}

int main()
{
    const int w = 44, h = 29, d = 35;   // partial bricks on every axis
    const float3 lo = make_float3(0.0f, 0.0f, 0.0f), hi = make_float3(43 / 16.0f, 28 / 16.0f, 34 / 16.0f);
    BoundedVolume<SDF_t, TargetDevice, Manage> vol(w, h, d, lo, hi);
    SdfSphere(vol, make_float3(0.5f, 0.9f, 1.0f), 1.15f);   // leaves the frame through five of its faces
    GpuCheckStatus(kfx_stream_synchronize(0));
    std::vector<SDF_t> cells((size_t)w * h * d);
    const size_t row = w * sizeof(SDF_t);
    GpuCheckStatus(kfx_memcpy_2d(cells.data(), row, vol.ptr, vol.pitch, row, (size_t)h * d, 2, 0));
    for (int z = 0; z < d; ++z)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                if ((x + y + z) % 7 == 0) cells[((size_t)z * h + y) * w + x].val = NAN;   // unobserved cells through the band
    vol.MemcpyFromHost(cells.data());

    Image<unsigned char, TargetDevice, Manage> scratch(BrickScratchBytes(vol), 1);
    const size_t n = BrickPlan(vol, NAN, scratch.ptr, scratch.w);
    CHECK(n == 6 * 4 * 5);
    Image<unsigned, TargetDevice, Manage> ids(n, 1);
    Image<unsigned char, TargetDevice, Manage> packed(n * BrickBytes(vol), 1);
    BrickPack(vol, NAN, scratch.ptr, scratch.w, n, ids.ptr, packed.ptr);
    std::vector<unsigned> host_ids(n);
    GpuCheckStatus(kfx_memcpy_2d(host_ids.data(), n * 4, ids.ptr, n * 4, n * 4, 1, 2, 0));

    const kfx_volume frame = BrickFrame(w, h, d, lo, hi);
    const ImageIntrinsics K(120.0f, 120.0f, (W - 1) / 2.0f, (H - 1) / 2.0f);
    Mat<float,3,4> T_a = SE3Identity(), T_b = SE3Identity();
    T_a(0, 3) = 1.3f; T_a(1, 3) = 0.9f; T_a(2, 3) = -2.0f;
    const float a = -1.0f;   // rot_y(-1 rad), looking back at the sphere from beyond the frame's +x face
    T_b(0, 0) = cosf(a); T_b(0, 2) = sinf(a); T_b(2, 0) = -sinf(a); T_b(2, 2) = cosf(a);
    T_b(0, 3) = 2.4f; T_b(1, 3) = 0.9f; T_b(2, 3) = 0.2f;
    const float near = 0.1f, far = 10.0f, trunc = 0.25f;

    Targets got, want;
    Image<unsigned char, TargetDevice, Manage> plan(RaycastBricksScratchBytes(n), 1);
    CHECK(plan.w == RaycastBricksScratchBytes(n, 0) && RaycastBricksScratchBytes(n, 5) > plan.w);
    RaycastBricksPlan(frame, ids.ptr, n, plan.ptr, plan.w);
    RaycastSdfBricks(got.depth, got.norm, got.img, frame, KFX_CELL_F32, ids.ptr, packed.ptr, n, plan.ptr, plan.w, T_b, K, near, far, trunc, true);
    RaycastSdf(want.depth, want.norm, want.img, vol, T_b, K, near, far, trunc, true);
    const Views all_b = got.Read(), all_d = want.Read();
    CHECK(all_d.hits() >= FLOOR && (size_t)W * H - all_d.hits() >= FLOOR);
    CHECK(SameBits(all_b, all_d));

    // a fifth of the bricks dropped: the list is the front of a compacted copy; the comparator is the volume reset and the others unpacked
    std::vector<unsigned> half_ids;
    std::vector<unsigned char> all(n * BrickBytes(vol)), half;
    GpuCheckStatus(kfx_memcpy_2d(all.data(), all.size(), packed.ptr, all.size(), all.size(), 1, 2, 0));
    for (size_t k = 0; k < n; ++k) {
        const unsigned id = host_ids[k], bx = id % 6, by = (id / 6) % 4, bz = id / 24;
        if ((bx + 2 * by + 3 * bz) % 5 == 0) continue;
        half_ids.push_back(host_ids[k]);
        half.insert(half.end(), all.begin() + k * BrickBytes(vol), all.begin() + (k + 1) * BrickBytes(vol));
    }
    const size_t m = half_ids.size();
    CHECK(m == n - 24);
    GpuCheckStatus(kfx_memcpy_2d(ids.ptr, m * 4, half_ids.data(), m * 4, m * 4, 1, 1, 0));
    GpuCheckStatus(kfx_memcpy_2d(packed.ptr, half.size(), half.data(), half.size(), half.size(), 1, 1, 0));
    SdfReset(vol, NAN);
    BrickUnpack(vol, ids.ptr, packed.ptr, m);
    RaycastBricksPlan(frame, ids.ptr, m, plan.ptr, plan.w);   // (the scratch of n entries is large enough for m)
    const Mat<float,3,4> poses[2] = {T_b, T_a};
    for (int k = 0; k < 2; ++k) {
        RaycastSdfBricks(got.depth, got.norm, got.img, frame, KFX_CELL_F32, ids.ptr, packed.ptr, m, plan.ptr, plan.w, poses[k], K, near, far, trunc, true);
        RaycastSdf(want.depth, want.norm, want.img, vol, poses[k], K, near, far, trunc, true);
        const Views fewer_b = got.Read(), fewer_d = want.Read();
        if (k == 0) CHECK(fewer_d.hits() >= FLOOR && (size_t)W * H - fewer_d.hits() >= FLOOR && !SameBits(fewer_d, all_d) && fewer_d.hits() < all_d.hits());
        CHECK(SameBits(fewer_b, fewer_d));

        // the colour overload, no colour bricks: 0.5 at every hit, 0 elsewhere
        RaycastSdfBricks(got.depth, got.norm, got.img, frame, ids.ptr, packed.ptr, m, nullptr, nullptr, 0, plan.ptr, plan.w, poses[k], K, near, far, trunc, true);
        const Views grey = got.Read();
        CHECK(SameBits(grey, fewer_d, false));
        size_t bad = 0;
        for (size_t px = 0; px < grey.d.size(); ++px) bad += grey.i[px] != (grey.d[px] > 0 ? 0.5f : 0.0f);
        CHECK(bad == 0);
    }

    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("passed\n");
    return 0;
}
