// roo_mesh_simplify_test.cpp -- roo::MeshSimplify and the `cell` argument of roo::SaveMeshIndexed from C++
// (include/kangaroo/MarchingCubes.h over include/kfx_mesh_simplify.h) on the three-sphere volume: 48^3 cells in [-1, 1]^3, the minimum
// of three sphere distances, V = 2480, T = 4948.
//   * MeshSimplify at cells of 2 and 4 voxel sizes and at 1/1024 of one against the contract restated on the host with std::map (the
//     same fp32 arithmetic, one operation at a time): rows of the representatives bit for bit, faces, the vertex map; the last returns
//     the input bit for bit; an origin that is not zero;
//   * SaveMeshIndexed(min_faces = 1000, largest = false, nvert, cell): the file holds the simplification of the filtered mesh; cell = 0
//     is the filtered file;
//   * a cell that is no length is refused.
// Prints "roo_mesh_simplify_test: ok" and exits 0 when every check holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include <unistd.h>

#include <kangaroo/kangaroo.h>

using namespace roo;

static int g_fail = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { ++g_fail; fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

typedef BoundedVolume<SDF_t, TargetDevice, Manage> Vol;

static void ToHost(std::vector<SDF_t>& out, const Vol& v)
{
    const size_t row = v.w * sizeof(SDF_t);
    out.resize((size_t)v.w * v.h * v.d);
    GpuCheckStatus(kfx_memcpy_2d(out.data(), row, v.ptr, v.pitch, row, (size_t)v.h * v.d, 2, 0));
}

static mesh_detail::DeviceBuffer Upload(const void* host, size_t bytes)
{
    mesh_detail::DeviceBuffer d(bytes);
    if (bytes) GpuCheckStatus(kfx_memcpy_2d(d.get(), bytes, host, bytes, bytes, 1, 1, 0));
    return d;
}

// the contract of include/kfx_mesh_simplify.h on host arrays
static mesh_detail::HostMesh Simplified(const mesh_detail::HostMesh& in, float cell, const float origin[3], std::vector<uint32_t>& vertex_cluster)
{
    const float inv = 1.0f / cell;
    const size_t V = in.nvert, T = in.ntri;
    std::map<std::tuple<long, long, long>, std::pair<uint32_t, uint32_t>> best;   // cell -> {d2 bits, id}
    std::vector<std::tuple<long, long, long>> cell_of(V);
    std::vector<uint32_t> rep(V);
    for (uint32_t v = 0; v < V; ++v) {
        long i[3];
        float t[3];
        bool single = false;
        for (int k = 0; k < 3; ++k) {
            const float d = in.v[3 * v + k] - origin[k];
            const float q = d * inv;
            const float fl = floorf(q);
            if (!std::isfinite(q) || fl < -1048576.0f || fl >= 1048576.0f) single = true;
            i[k] = single ? 0 : (long)fl;
            const float r = q - fl;
            t[k] = r - 0.5f;
        }
        const float xx = t[0] * t[0], yy = t[1] * t[1], zz = t[2] * t[2];
        const float xy = xx + yy;
        const float d2 = xy + zz;
        uint32_t bits;
        memcpy(&bits, &d2, 4);
        cell_of[v] = single ? std::make_tuple(1L << 40, (long)v, 0L) : std::make_tuple(i[0], i[1], i[2]);
        const std::pair<uint32_t, uint32_t> me(single ? 0u : bits, v);
        auto it = best.find(cell_of[v]);
        if (it == best.end() || me < it->second) best[cell_of[v]] = me;
    }
    for (uint32_t v = 0; v < V; ++v) rep[v] = best[cell_of[v]].second;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, size_t> first;
    std::vector<char> keep(T, 0), used(V, 0);
    for (size_t f = 0; f < T; ++f) {
        uint32_t c[3] = {rep[in.faces[3 * f]], rep[in.faces[3 * f + 1]], rep[in.faces[3 * f + 2]]};
        if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) continue;
        std::sort(c, c + 3);
        if (first.emplace(std::make_tuple(c[0], c[1], c[2]), f).second) {
            keep[f] = 1;
            used[c[0]] = used[c[1]] = used[c[2]] = 1;
        }
    }
    mesh_detail::HostMesh out;
    std::vector<uint32_t> remap(V, 0xffffffffu);
    for (uint32_t v = 0; v < V; ++v)
        if (used[v]) {
            remap[v] = (uint32_t)out.nvert++;
            out.v.insert(out.v.end(), &in.v[3 * v], &in.v[3 * v] + 3);
            out.n.insert(out.n.end(), &in.n[3 * v], &in.n[3 * v] + 3);
        }
    vertex_cluster.resize(V);
    for (uint32_t v = 0; v < V; ++v) vertex_cluster[v] = remap[rep[v]];
    for (size_t f = 0; f < T; ++f)
        if (keep[f]) {
            for (int k = 0; k < 3; ++k) out.faces.push_back(remap[rep[in.faces[3 * f + k]]]);
            ++out.ntri;
        }
    return out;
}

static bool Same(const mesh_detail::HostMesh& a, const mesh_detail::HostMesh& b)
{
    return a.nvert == b.nvert && a.ntri == b.ntri && a.faces == b.faces && a.v.size() == b.v.size() && a.n.size() == b.n.size() &&
           !memcmp(a.v.data(), b.v.data(), a.v.size() * 4) && !memcmp(a.n.data(), b.n.data(), a.n.size() * 4);
}

static std::vector<unsigned char> ReadFile(const std::string& path)
{
    std::vector<unsigned char> b;
    if (FILE* f = fopen(path.c_str(), "rb")) {
        unsigned char buf[1 << 16];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
        fclose(f);
    }
    return b;
}

// whether the PLY at `path` holds exactly `want`
static bool FileHolds(const std::string& path, const mesh_detail::HostMesh& want)
{
    const std::vector<unsigned char> b = ReadFile(path);
    const char* end = "end_header\n";
    const auto it = std::search(b.begin(), b.end(), end, end + strlen(end));
    if (it == b.end()) return false;
    const size_t body = (size_t)(it - b.begin()) + strlen(end);
    bool rows = b.size() == body + 24 * want.nvert + 13 * want.ntri;
    for (size_t v = 0; rows && v < want.nvert; ++v)
        rows = !memcmp(&b[body + 24 * v], &want.v[3 * v], 12) && !memcmp(&b[body + 24 * v + 12], &want.n[3 * v], 12);
    for (size_t t = 0; rows && t < want.ntri; ++t)
        rows = b[body + 24 * want.nvert + 13 * t] == 3 && !memcmp(&b[body + 24 * want.nvert + 13 * t + 1], &want.faces[3 * t], 12);
    return rows;
}

int main()
{
    if (kfx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    const std::string tmp = "/tmp/roo_mesh_simplify_test." + std::to_string((long)getpid());
    const BoundingBox bb(make_float3(-1.0f, -1.0f, -1.0f), make_float3(1.0f, 1.0f, 1.0f));
    const size_t N = 48;
    const float voxel = 2.0f / 48.0f;
    Vol vol(N, N, N, bb), other(N, N, N, bb);
    {
        std::vector<SDF_t> least, part;
        SdfSphere(vol, make_float3(-0.45f, -0.1f, 0.0f), 0.35f);
        ToHost(least, vol);
        const float3 centres[2] = {make_float3(0.45f, 0.1f, 0.05f), make_float3(0.0f, 0.7f, 0.6f)};
        const float radii[2] = {0.33f, 0.08f};
        for (int s = 0; s < 2; ++s) {
            SdfSphere(other, centres[s], radii[s]);
            ToHost(part, other);
            for (size_t i = 0; i < least.size(); ++i) least[i].val = std::min(least[i].val, part[i].val);
        }
        vol.MemcpyFromHost(least.data());
    }

    // the indexed mesh, as host arrays and again in device memory
    const mesh_detail::HostMesh m = mesh_detail::Extract(vol.abi(), KFX_CELL_F32, nullptr, 0, 0, nullptr, true);
    CHECK(m.nvert == 2480 && m.ntri == 4948);
    const mesh_detail::DeviceBuffer dv = Upload(m.v.data(), m.v.size() * 4), dn = Upload(m.n.data(), m.n.size() * 4), df = Upload(m.faces.data(), m.faces.size() * 4);
    const float zero[3] = {0.0f, 0.0f, 0.0f}, moved[3] = {0.013f, -0.4f, 7.0f};

    // ---- MeshSimplify ----
    for (const float cells : {2.0f, 4.0f, 1.0f / 1024.0f})
        for (const float* origin : {zero, moved}) {
            std::vector<uint32_t> map, want_map;
            const mesh_detail::HostMesh got = MeshSimplify(dv.get<float>(), dn.get<float>(), nullptr, df.get<uint32_t>(), m.nvert, m.ntri, cells * voxel, origin, &map);
            const mesh_detail::HostMesh want = Simplified(m, cells * voxel, origin, want_map);
            CHECK(Same(got, want) && map == want_map && !got.color && got.c.empty());
            if (cells >= 1.0f) CHECK(got.ntri > 0 && got.ntri < m.ntri && got.nvert > 0 && got.nvert < m.nvert);
            else CHECK(Same(got, m));
        }
    {
        const mesh_detail::HostMesh plain = MeshSimplify(dv.get<float>(), nullptr, nullptr, df.get<uint32_t>(), m.nvert, m.ntri, 2 * voxel);
        std::vector<uint32_t> want_map;
        const mesh_detail::HostMesh want = Simplified(m, 2 * voxel, zero, want_map);
        CHECK(plain.ntri == 1006 && plain.nvert == want.nvert && plain.n.empty() && plain.faces == want.faces && !memcmp(plain.v.data(), want.v.data(), want.v.size() * 4));
    }

    // ---- SaveMeshIndexed(min_faces, largest, nvert, cell): the simplification of the filtered mesh in the file ----
    {
        size_t nvert = 0;
        std::vector<uint32_t> unused;
        const mesh_detail::HostMesh filtered = mesh_detail::Extract(vol.abi(), KFX_CELL_F32, nullptr, 0, 0, nullptr, true, mesh_detail::MeshKeep{1000, false});
        CHECK(filtered.nvert == 2412 && filtered.ntri == 4816);
        const mesh_detail::HostMesh want = Simplified(filtered, 2 * voxel, zero, unused);
        CHECK(SaveMeshIndexed(tmp, vol, 1000, false, &nvert, 2 * voxel) == want.ntri && nvert == want.nvert && want.ntri > 0 && want.ntri < 4816);
        CHECK(FileHolds(tmp + ".ply", want));
        const mesh_detail::HostMesh all = Simplified(m, 4 * voxel, zero, unused);
        CHECK(SaveMeshIndexed(tmp, vol, 0, false, &nvert, 4 * voxel) == all.ntri && nvert == all.nvert && FileHolds(tmp + ".ply", all));
        CHECK(SaveMeshIndexed(tmp, vol, 1000, false, &nvert, 0.0f) == 4816 && nvert == 2412 && FileHolds(tmp + ".ply", filtered));
        CHECK(SaveMeshIndexed(tmp, vol, 1000, false, &nvert) == 4816 && nvert == 2412);
        remove((tmp + ".ply").c_str());
    }

    // ---- a cell that is no length ----
    for (const float bad : {-1.0f, NAN, INFINITY}) {
        const size_t nbytes = kfx_mesh_simplify_scratch_bytes(m.nvert, m.ntri);
        mesh_detail::DeviceBuffer scratch(nbytes);
        unsigned long long kept[2] = {7, 7};
        CHECK(kfx_mesh_simplify_plan(dv.get<float>(), df.get<unsigned>(), m.ntri, m.nvert, zero, bad, scratch.get(), nbytes, kept, 0) == KFX_E_RANGE);
        CHECK(kept[0] == 7 && kept[1] == 7);
    }

    if (g_fail) {
        printf("roo_mesh_simplify_test: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("roo_mesh_simplify_test: ok\n");
    return 0;
}
