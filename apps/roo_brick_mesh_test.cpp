// roo_brick_mesh_test.cpp -- roo::MeshBricksPlan / MeshBricksEmit / SaveMeshBricks from C++ (include/kangaroo/VolumeBricks.h over
// include/kfx_mesh_bricks.h): a small volume with a sphere and some unobserved cells is packed into bricks, the bricks are meshed, the
// volume is meshed (roo::SaveMesh's extraction, include/kfx_mesh.h), and the two are compared cube by cube:
//   * the brick mesh lists the dense mesh's cubes, brick by brick, ascending within a brick;
//   * every cube has the same triangles: vertex and normal bits;
//   * with half of the bricks left out, the brick mesh is the dense mesh of the volume those bricks unpack into;
//   * SaveMeshBricks writes a PLY with the triangle count.
// Prints "passed" and exits 0 when every check holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include <kangaroo/kangaroo.h>
#include <kangaroo/VolumeBricks.h>

using namespace roo;

static int g_fail = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { ++g_fail; fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

struct Soup {
    mesh_detail::HostMesh m;
    std::vector<long long> ci;
    std::vector<unsigned> to;
};

// the dense soup with its cube list (kfx_mesh_plan / kfx_mesh_emit)
static Soup Dense(const BoundedVolume<SDF_t, TargetDevice, Manage>& vol)
{
    Soup s;
    const size_t nbytes = kfx_mesh_scratch_bytes(vol.abi(), KFX_CELL_F32, nullptr, 0, 0);
    mesh_detail::DeviceBuffer scratch(nbytes);
    unsigned long long totals[2] = {0, 0};
    GpuCheckStatus(kfx_mesh_plan(vol.abi(), KFX_CELL_F32, nullptr, 0, 0, scratch.get(), nbytes, totals, 0));
    const size_t na = totals[0], nv = 3 * totals[1];
    mesh_detail::DeviceBuffer active(na * 8), offsets(na * 4), dv(nv * 12), dn(nv * 12);
    if (na)
        GpuCheckStatus(kfx_mesh_emit(vol.abi(), KFX_CELL_F32, nullptr, 0, 0, nullptr, scratch.get(), nbytes, totals, active.get<long long>(),
                                     offsets.get<unsigned>(), dv.get<float>(), dn.get<float>(), nullptr, 0));
    s.m.ntri = totals[1]; s.m.nvert = nv;
    s.m.v.resize(nv * 3); s.m.n.resize(nv * 3); s.ci.resize(na); s.to.resize(na);
    dv.CopyTo(s.m.v.data(), nv * 12); dn.CopyTo(s.m.n.data(), nv * 12);
    active.CopyTo(s.ci.data(), na * 8); offsets.CopyTo(s.to.data(), na * 4);
    return s;
}

// brick soup against dense soup, by cube; w, h, d: the frame
static void Compare(const Soup& b, const Soup& dn, int w, int h, int d, const std::vector<unsigned>& ids)
{
    CHECK(b.ci.size() == dn.ci.size() && b.m.ntri == dn.m.ntri && dn.ci.size() > 100);
    if (b.ci.size() != dn.ci.size() || b.m.ntri != dn.m.ntri) return;
    const int nbx = (w + 7) / 8, nby = (h + 7) / 8;
    long long prev_brick = -1, prev_ci = -1;
    size_t order_bad = 0, cube_bad = 0, bits_bad = 0;
    for (size_t k = 0; k < b.ci.size(); ++k) {
        const long long ci = b.ci[k];
        const int z = (int)(ci % (d - 1)), y = (int)((ci / (d - 1)) % (h - 1)), x = (int)(ci / ((long long)(d - 1) * (h - 1)));
        const long long brick = ((long long)(z >> 3) * nby + (y >> 3)) * nbx + (x >> 3);
        order_bad += brick < prev_brick || (brick == prev_brick && ci <= prev_ci) || !std::binary_search(ids.begin(), ids.end(), (unsigned)brick);
        prev_brick = brick; prev_ci = ci;
        const size_t j = std::lower_bound(dn.ci.begin(), dn.ci.end(), ci) - dn.ci.begin();
        if (j >= dn.ci.size() || dn.ci[j] != ci) { ++cube_bad; continue; }
        const size_t nb = (k + 1 < b.to.size() ? b.to[k + 1] : b.m.ntri) - b.to[k], nd = (j + 1 < dn.to.size() ? dn.to[j + 1] : dn.m.ntri) - dn.to[j];
        if (nb != nd) { ++cube_bad; continue; }
        bits_bad += memcmp(&b.m.v[(size_t)b.to[k] * 9], &dn.m.v[(size_t)dn.to[j] * 9], nb * 36) != 0;
        bits_bad += memcmp(&b.m.n[(size_t)b.to[k] * 9], &dn.m.n[(size_t)dn.to[j] * 9], nb * 36) != 0;
    }
    if (order_bad || cube_bad || bits_bad) fprintf(stderr, "%zu cubes out of order, %zu cubes differ, %zu cubes with other bits\n", order_bad, cube_bad, bits_bad);
    CHECK(order_bad == 0 && cube_bad == 0 && bits_bad == 0);
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
    Soup bricks;
    bricks.m = mesh_detail::ExtractBricks(frame, KFX_CELL_F32, ids.ptr, packed.ptr, n, nullptr, nullptr, 0, false, false, &bricks.ci, &bricks.to);
    Compare(bricks, Dense(vol), w, h, d, host_ids);

    // every other brick: the list is the front of a compacted copy; the comparator is the volume reset and those bricks unpacked
    std::vector<unsigned> half_ids;
    std::vector<unsigned char> all(n * BrickBytes(vol)), half;
    GpuCheckStatus(kfx_memcpy_2d(all.data(), all.size(), packed.ptr, all.size(), all.size(), 1, 2, 0));
    for (size_t k = 0; k < n; k += 2) {
        half_ids.push_back(host_ids[k]);
        half.insert(half.end(), all.begin() + k * BrickBytes(vol), all.begin() + (k + 1) * BrickBytes(vol));
    }
    const size_t m = half_ids.size();
    GpuCheckStatus(kfx_memcpy_2d(ids.ptr, m * 4, half_ids.data(), m * 4, m * 4, 1, 1, 0));
    GpuCheckStatus(kfx_memcpy_2d(packed.ptr, half.size(), half.data(), half.size(), half.size(), 1, 1, 0));
    SdfReset(vol, NAN);
    BrickUnpack(vol, ids.ptr, packed.ptr, m);
    Soup fewer;
    fewer.m = mesh_detail::ExtractBricks(frame, KFX_CELL_F32, ids.ptr, packed.ptr, m, nullptr, nullptr, 0, false, false, &fewer.ci, &fewer.to);
    CHECK(fewer.ci.size() < bricks.ci.size());
    Compare(fewer, Dense(vol), w, h, d, half_ids);

    const size_t ntri = SaveMeshBricks("/tmp/roo_brick_mesh_test", frame, KFX_CELL_F32, ids.ptr, packed.ptr, m);
    CHECK(ntri == fewer.m.ntri && ntri > 0);
    if (FILE* f = fopen("/tmp/roo_brick_mesh_test.ply", "rb")) {
        char head[256] = {0};
        CHECK(fread(head, 1, 255, f) > 0 && strstr(head, "element vertex") != nullptr);
        fclose(f);
        remove("/tmp/roo_brick_mesh_test.ply");
    } else {
        CHECK(!"the PLY was not written");
    }
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("passed\n");
    return 0;
}
