// roo_half_summary_test.cpp -- the brick summary of a half-cell volume (roo::SdfSummary on BoundedVolume<SDF_h>, config C5) from C++:
// the tracked SdfReset / SdfFuse / RaycastSdf / RaycastSdfLevels overloads of include/kangaroo/SdfSummary.h against the plain SDF_h
// calls, exact numerics.  The volume must be bit-identical and every image bit-identical, also on a view at multiples of 8 cells
// and after Rebuild / Invalidate.  Prints "passed" and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <kangaroo/kangaroo.h>
#include <kangaroo/SdfSummary.h>

using namespace roo;

static int g_fail = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { ++g_fail; fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static bool same(float a, float b) { return (a == b) || (std::isnan(a) && std::isnan(b)); }

template <typename T>
static std::vector<T> host(const Image<T, TargetDevice, Manage>& im)
{
    std::vector<T> v((size_t)im.w * im.h);
    im.MemcpyToHost(v.data());
    return v;
}

// bit-identical images (depth, normal, shade); returns the number of hits
static int compare(const Image<float, TargetDevice, Manage>& da, const Image<float4, TargetDevice, Manage>& na, const Image<float, TargetDevice, Manage>& ia,
                   const Image<float, TargetDevice, Manage>& db, const Image<float4, TargetDevice, Manage>& nb, const Image<float, TargetDevice, Manage>& ib)
{
    const std::vector<float> hda = host(da), hdb = host(db), hia = host(ia), hib = host(ib);
    const std::vector<float4> hna = host(na), hnb = host(nb);
    int hits = 0, bad = 0;
    for (size_t i = 0; i < hda.size(); ++i) {
        if (std::isfinite(hda[i])) ++hits;
        if (!same(hda[i], hdb[i]) || !same(hia[i], hib[i]) || !same(hna[i].x, hnb[i].x) || !same(hna[i].y, hnb[i].y) ||
            !same(hna[i].z, hnb[i].z) || !same(hna[i].w, hnb[i].w))
            ++bad;
    }
    CHECK(bad == 0);
    return hits;
}

template <typename M1, typename M2>
static bool same_volume(const BoundedVolume<SDF_h, TargetDevice, M1>& a, const BoundedVolume<SDF_h, TargetDevice, M2>& b)
{
    const size_t row = a.w * sizeof(SDF_h);
    std::vector<unsigned char> ha(row * a.h * a.d), hb(row * a.h * a.d);
    CHECK(kfx_memcpy_2d(ha.data(), row, a.ptr, a.pitch, row, (size_t)a.h * a.d, 2, 0) == 0);
    CHECK(kfx_memcpy_2d(hb.data(), row, b.ptr, b.pitch, row, (size_t)b.h * b.d, 2, 0) == 0);
    return memcmp(ha.data(), hb.data(), ha.size()) == 0;
}

int main()
{
    if (kfx_device_count() < 1) {
        printf("roo_half_summary_test: no HIP device\n");
        return 1;
    }
    kfx_set_math_mode(KFX_MATH_EXACT);
    const int M = 64, sw = 160, sh = 120;
    const ImageIntrinsics Ks(142.5855, 142.5855, sw / 2.0 - 0.5, sh / 2.0 - 0.5);
    const BoundingBox box(make_float3(-1, -1, 2), make_float3(1, 1, 4));
    BoundedVolume<SDF_h, TargetDevice, Manage> va(M, M, M, box), vb(M, M, M, box);
    Image<float, TargetDevice, Manage> sd(sw, sh), da(sw, sh), db(sw, sh), ia(sw, sh), ib(sw, sh);
    Image<float4, TargetDevice, Manage> sv(sw, sh), sn(sw, sh), na(sw, sh), nb(sw, sh);
    std::vector<float> wall((size_t)sw * sh, 3.5f);
    for (int v = 30; v < 90; ++v)
        for (int u = 40; u < 120; ++u) wall[(size_t)v * sw + u] = 2.8f + 0.001f * (float)((u * 7 + v * 3) % 11);   // a box in front of the wall
    sd.MemcpyFromHost(wall.data());
    DepthToVbo<float>(sv, sd, Ks);
    NormalsFromVbo(sn, sv);
    const float tr = 2.0f * length(va.VoxelSizeUnits());

    SdfSummary summary(vb);
    SdfReset(va, NAN);
    SdfReset(vb, NAN, summary);
    Mat<float,3,4> T = SE3Identity();
    int hits = 0;
    for (int f = 0; f < 3; ++f) {
        T(0, 3) = 0.01f * (float)f;
        const Mat<float,3,4> Tinv = SE3inv(T);
        SdfFuse(va, sd, sn, Tinv, Ks, tr, 1000.0f, 0.1f);
        SdfFuse(vb, summary, sd, sn, Tinv, Ks, tr, 1000.0f, 0.1f);
        CHECK(same_volume(va, vb));   // tracking only observes
        RaycastSdf(da, na, ia, va, T, Ks, 0.4f, 8.0f, tr, true);
        RaycastSdf(db, nb, ib, vb, summary, T, Ks, 0.4f, 8.0f, tr, true);
        hits = compare(da, na, ia, db, nb, ib);
        CHECK(hits > sw * sh / 4);
    }

    // a view at multiples of 8 cells: tracked SdfFuse on it keeps the parent's summary current
    {
        const int o = 8, n = 48;
        BoundedVolume<SDF_h, TargetDevice, DontManage> wa = va.SubBoundingVolume(BoundingBox(va.VoxelPositionInUnits(o, o, o), va.VoxelPositionInUnits(o + n - 1, o + n - 1, o + n - 1)));
        BoundedVolume<SDF_h, TargetDevice, DontManage> wb = vb.SubBoundingVolume(BoundingBox(vb.VoxelPositionInUnits(o, o, o), vb.VoxelPositionInUnits(o + n - 1, o + n - 1, o + n - 1)));
        T(0, 3) = -0.01f;
        const Mat<float,3,4> Tinv = SE3inv(T);
        SdfFuse(wa, sd, sn, Tinv, Ks, tr, 1000.0f, 0.1f);
        SdfFuse(wb, summary, sd, sn, Tinv, Ks, tr, 1000.0f, 0.1f);
        CHECK(same_volume(va, vb));
        RaycastSdf(da, na, ia, va, T, Ks, 0.4f, 8.0f, tr, true);
        RaycastSdf(db, nb, ib, vb, summary, T, Ks, 0.4f, 8.0f, tr, true);
        CHECK(compare(da, na, ia, db, nb, ib) > sw * sh / 4);
    }

    // the pyramid levels of the tracking loop in one tracked launch against per-level plain calls
    {
        Image<float, TargetDevice, Manage> ld[3] = {Image<float, TargetDevice, Manage>(sw, sh), Image<float, TargetDevice, Manage>(sw / 4, sh / 4),
                                                    Image<float, TargetDevice, Manage>(sw / 8, sh / 8)};
        Image<float, TargetDevice, Manage> li[3] = {Image<float, TargetDevice, Manage>(sw, sh), Image<float, TargetDevice, Manage>(sw / 4, sh / 4),
                                                    Image<float, TargetDevice, Manage>(sw / 8, sh / 8)};
        Image<float4, TargetDevice, Manage> ln[3] = {Image<float4, TargetDevice, Manage>(sw, sh), Image<float4, TargetDevice, Manage>(sw / 4, sh / 4),
                                                     Image<float4, TargetDevice, Manage>(sw / 8, sh / 8)};
        Image<float> d3[3] = {ld[0], ld[1], ld[2]}, i3[3] = {li[0], li[1], li[2]};
        Image<float4> n3[3] = {ln[0], ln[1], ln[2]};
        const ImageIntrinsics K3[3] = {Ks, ImageIntrinsics(Ks.fu / 4, Ks.fv / 4, (Ks.u0 + 0.5f) / 4 - 0.5f, (Ks.v0 + 0.5f) / 4 - 0.5f),
                                       ImageIntrinsics(Ks.fu / 8, Ks.fv / 8, (Ks.u0 + 0.5f) / 8 - 0.5f, (Ks.v0 + 0.5f) / 8 - 0.5f)};
        RaycastSdfLevels(d3, n3, i3, 3, vb, summary, T, K3, 0.4f, 8.0f, tr, true);
        for (int l = 0; l < 3; ++l) {
            Image<float, TargetDevice, Manage> pd(ld[l].w, ld[l].h), pi(ld[l].w, ld[l].h);
            Image<float4, TargetDevice, Manage> pn(ld[l].w, ld[l].h);
            RaycastSdf(pd, pn, pi, va, T, K3[l], 0.4f, 8.0f, tr, true);
            compare(pd, pn, pi, ld[l], ln[l], li[l]);
        }
    }

    // writers that do not track: Rebuild (exact ranges) and Invalidate (nothing known) keep the images those of the plain march
    SdfSphere(va, make_float3(0.f, 0.f, 3.f), 0.3f);
    SdfSphere(vb, make_float3(0.f, 0.f, 3.f), 0.3f);
    summary.Rebuild();
    RaycastSdf(da, na, ia, va, T, Ks, 0.4f, 8.0f, tr, true);
    RaycastSdf(db, nb, ib, vb, summary, T, Ks, 0.4f, 8.0f, tr, true);
    hits = compare(da, na, ia, db, nb, ib);
    summary.Invalidate();
    RaycastSdf(db, nb, ib, vb, summary, T, Ks, 0.4f, 8.0f, tr, true);
    compare(da, na, ia, db, nb, ib);

    // an fp32 summary is refused by the half calls (KFX_E_SHAPE), and the volume is left as it was
    {
        BoundedVolume<SDF_t, TargetDevice, Manage> v32(M, M, M, box);
        SdfSummary s32(v32);
        CHECK(kfx_sdf_fuse_tracked_h(vb.abi(), s32.get(), sd.abi(), sn.abi(), SE3Identity().m, &Ks.fu, tr, 1000.0f, 0.1f, 0, 0) == KFX_E_SHAPE);
        CHECK(same_volume(va, vb));
    }

    printf("roo_half_summary_test: %s (%d ray hits checked)\n", g_fail ? "FAILED" : "passed", hits);
    return g_fail ? 1 : 0;
}
