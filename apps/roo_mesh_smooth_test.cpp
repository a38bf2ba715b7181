// roo_mesh_smooth_test.cpp -- roo::MeshAdjacency, roo::MeshSmooth, roo::MeshVertexNormals and the `smooth_iterations` argument of
// roo::SaveMeshIndexed from C++ (include/kangaroo/MarchingCubes.h over include/kfx_mesh_smooth.h) on the three-sphere volume: 48^3 cells
// in [-1, 1]^3, the minimum of three sphere distances, V = 2480, T = 4948, closed.
//   * MeshAdjacency against the contract restated on the host (every vertex's corner slots in ascending order; no flag on a closed
//     manifold mesh);
//   * MeshSmooth with 0, 1 and 5 Taubin iterations and one plain Laplacian pass, and MeshVertexNormals of the result, against the
//     contract restated on the host (the same fp32 arithmetic, one operation at a time), bit for bit; every recomputed normal of the
//     unsmoothed mesh lies on the side of the extraction's;
//   * SaveMeshIndexed(min_faces, largest, nvert, cell, smooth_iterations): the file holds the smoothing of the filtered mesh, colours
//     absent; smooth_iterations = 0 is the filtered file;
//   * parameters out of range are refused.
// Prints "roo_mesh_smooth_test: ok" and exits 0 when every check holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
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

// the contract of include/kfx_mesh_smooth.h on host arrays
struct HostAdjacency {
    std::vector<uint32_t> start, inc, flags;
};
static HostAdjacency Adjacency(const std::vector<uint32_t>& faces, size_t V)
{
    HostAdjacency a;
    a.start.assign(V + 1, 0);
    for (uint32_t id : faces) ++a.start[id + 1];
    for (size_t v = 0; v < V; ++v) a.start[v + 1] += a.start[v];
    std::vector<uint32_t> at(a.start.begin(), a.start.end() - 1);
    a.inc.resize(faces.size());
    for (uint32_t s = 0; s < faces.size(); ++s) a.inc[at[faces[s]]++] = s;   // (ascending s: the lists ascend)
    a.flags.assign(V, 0);
    for (uint32_t v = 0; v < V; ++v) {
        std::vector<uint32_t> u;
        for (uint32_t i = a.start[v]; i < a.start[v + 1]; ++i) {
            const uint32_t s = a.inc[i], f = s / 3, c = s % 3;
            u.push_back(faces[3 * f + (c + 1) % 3]);
            u.push_back(faces[3 * f + (c + 2) % 3]);
        }
        if (u.empty()) a.flags[v] |= KFX_MESH_ISOLATED;
        for (uint32_t x : u) {
            const size_t cnt = (size_t)std::count(u.begin(), u.end(), x);
            if (x == v) a.flags[v] |= KFX_MESH_DEGENERATE;
            else if (cnt == 1) a.flags[v] |= KFX_MESH_BOUNDARY;
            else if (cnt > 2) a.flags[v] |= KFX_MESH_NONMANIFOLD;
        }
    }
    return a;
}

static std::vector<float> Smoothed(std::vector<float> p, const std::vector<uint32_t>& faces, const HostAdjacency& a, const mesh_detail::MeshSmoothing& how)
{
    const size_t V = p.size() / 3;
    for (int pass = 0; pass < 2 * how.iterations; ++pass) {
        const float factor = pass % 2 ? how.mu : how.lambda;
        if (pass % 2 && how.mu == 0.0f) continue;
        std::vector<float> o = p;
        for (uint32_t v = 0; v < V; ++v) {
            const uint32_t d = a.start[v + 1] - a.start[v];
            if (!d || (how.pin_boundary && (a.flags[v] & KFX_MESH_BOUNDARY))) continue;
            volatile float acc[3] = {0.0f, 0.0f, 0.0f};
            for (uint32_t i = a.start[v]; i < a.start[v + 1]; ++i) {
                const uint32_t s = a.inc[i], f = s / 3, c = s % 3;
                for (int e = 1; e <= 2; ++e)
                    for (int k = 0; k < 3; ++k) acc[k] = acc[k] + p[3 * faces[3 * f + (c + e) % 3] + k];
            }
            float r[3];
            bool finite = true;
            for (int k = 0; k < 3; ++k) {
                volatile float mean = acc[k] / (float)(2 * d);
                volatile float dk = mean - p[3 * v + k];
                volatile float step = factor * dk;
                r[k] = p[3 * v + k] + step;
                finite = finite && std::isfinite(r[k]);
            }
            if (finite) memcpy(&o[3 * v], r, 12);
        }
        p.swap(o);
    }
    return p;
}

static std::vector<float> Normals(const std::vector<float>& p, const std::vector<uint32_t>& faces, const HostAdjacency& a)
{
    const size_t V = p.size() / 3;
    std::vector<float> out(3 * V, 0.0f);
    for (uint32_t v = 0; v < V; ++v) {
        volatile float acc[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t i = a.start[v]; i < a.start[v + 1]; ++i) {
            const uint32_t* const id = &faces[3 * (a.inc[i] / 3)];
            volatile float e1[3], e2[3];
            for (int k = 0; k < 3; ++k) {
                e1[k] = p[3 * id[1] + k] - p[3 * id[0] + k];
                e2[k] = p[3 * id[2] + k] - p[3 * id[0] + k];
            }
            for (int k = 0; k < 3; ++k) {   // e2 x e1
                volatile float left = e1[(k + 2) % 3] * e2[(k + 1) % 3], right = e1[(k + 1) % 3] * e2[(k + 2) % 3];
                volatile float term = left - right;
                acc[k] = acc[k] + term;
            }
        }
        volatile float xx = acc[0] * acc[0], yy = acc[1] * acc[1], zz = acc[2] * acc[2];
        volatile float xy = xx + yy;
        volatile float l2 = xy + zz;
        if (a.start[v + 1] == a.start[v] || !std::isfinite(l2) || !(l2 > 0.0f)) continue;
        const float l = sqrtf(l2);
        for (int k = 0; k < 3; ++k) out[3 * v + k] = acc[k] / l;
    }
    return out;
}

static bool SameBits(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && !memcmp(a.data(), b.data(), a.size() * 4); }

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
    const std::string tmp = "/tmp/roo_mesh_smooth_test." + std::to_string((long)getpid());
    const BoundingBox bb(make_float3(-1.0f, -1.0f, -1.0f), make_float3(1.0f, 1.0f, 1.0f));
    const size_t N = 48;
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
    const mesh_detail::DeviceBuffer dv = Upload(m.v.data(), m.v.size() * 4), df = Upload(m.faces.data(), m.faces.size() * 4);
    const HostAdjacency want_adj = Adjacency(m.faces, m.nvert);

    // ---- MeshAdjacency ----
    {
        std::vector<uint32_t> start, inc, flags;
        MeshAdjacency(df.get<uint32_t>(), m.ntri, m.nvert, start, inc, &flags);
        CHECK(start == want_adj.start && inc == want_adj.inc && flags == want_adj.flags);
        CHECK(std::count(flags.begin(), flags.end(), 0u) == (long)m.nvert);   // closed and manifold
        std::vector<uint32_t> start2, inc2;
        MeshAdjacency(df.get<uint32_t>(), m.ntri, m.nvert, start2, inc2);
        CHECK(start2 == start && inc2 == inc);
    }

    // ---- MeshSmooth and MeshVertexNormals ----
    {
        const std::vector<float> normals = MeshVertexNormals(dv.get<float>(), df.get<uint32_t>(), m.nvert, m.ntri);
        CHECK(SameBits(normals, Normals(m.v, m.faces, want_adj)));
        bool same_side = true;
        for (size_t v = 0; v < m.nvert; ++v)
            same_side = same_side && normals[3 * v] * m.n[3 * v] + normals[3 * v + 1] * m.n[3 * v + 1] + normals[3 * v + 2] * m.n[3 * v + 2] > 0.0f;
        CHECK(same_side);
    }
    for (const int iterations : {0, 1, 5})
        for (const float mu : {-0.53f, 0.0f}) {
            mesh_detail::MeshSmoothing how;
            how.iterations = iterations;
            how.mu = mu;
            how.pin_boundary = mu != 0.0f;
            std::vector<float> normals;
            const std::vector<float> got = MeshSmooth(dv.get<float>(), df.get<uint32_t>(), m.nvert, m.ntri, how, &normals);
            const std::vector<float> want = Smoothed(m.v, m.faces, want_adj, how);
            CHECK(SameBits(got, want) && SameBits(normals, Normals(want, m.faces, want_adj)));
            CHECK((iterations == 0) == SameBits(got, m.v));
        }

    // ---- SaveMeshIndexed(min_faces, largest, nvert, cell, smooth_iterations): the smoothing of the filtered mesh in the file ----
    {
        size_t nvert = 0;
        mesh_detail::HostMesh filtered = mesh_detail::Extract(vol.abi(), KFX_CELL_F32, nullptr, 0, 0, nullptr, true, mesh_detail::MeshKeep{1000, false});
        CHECK(filtered.nvert == 2412 && filtered.ntri == 4816);
        CHECK(SaveMeshIndexed(tmp, vol, 1000, false, &nvert, 0.0f, 0) == 4816 && nvert == 2412 && FileHolds(tmp + ".ply", filtered));
        const HostAdjacency a = Adjacency(filtered.faces, filtered.nvert);
        mesh_detail::MeshSmoothing how;
        how.iterations = 3;
        mesh_detail::HostMesh want = filtered;
        want.v = Smoothed(filtered.v, filtered.faces, a, how);
        want.n = Normals(want.v, filtered.faces, a);
        CHECK(SaveMeshIndexed(tmp, vol, 1000, false, &nvert, 0.0f, 3) == 4816 && nvert == 2412 && FileHolds(tmp + ".ply", want));
        CHECK(!SameBits(want.v, filtered.v));
        remove((tmp + ".ply").c_str());
    }

    // ---- parameters out of range ----
    {
        const mesh_detail::DeviceAdjacency a = mesh_detail::Adjacency(df.get<unsigned>(), m.nvert, m.ntri, true);
        const size_t nbytes = kfx_mesh_smooth_scratch_bytes(m.nvert, m.ntri);
        mesh_detail::DeviceBuffer scratch(nbytes), out(m.nvert * 12);
        const float bad[][2] = {{0.0f, -0.53f}, {1.5f, -0.53f}, {NAN, -0.53f}, {0.5f, 0.1f}, {0.5f, NAN}, {0.5f, -INFINITY}};
        for (const auto& b : bad)
            CHECK(kfx_mesh_smooth(dv.get<float>(), df.get<unsigned>(), m.ntri, m.nvert, a.start.get<unsigned>(), a.inc.get<unsigned>(), a.flags.get<unsigned>(), 1,
                                  b[0], b[1], 1u, out.get<float>(), scratch.get(), nbytes, 0) == KFX_E_RANGE);
        CHECK(kfx_mesh_smooth(dv.get<float>(), df.get<unsigned>(), m.ntri, m.nvert, a.start.get<unsigned>(), a.inc.get<unsigned>(), a.flags.get<unsigned>(), -1,
                              0.5f, -0.53f, 1u, out.get<float>(), scratch.get(), nbytes, 0) == KFX_E_RANGE);
    }

    if (g_fail) {
        printf("roo_mesh_smooth_test: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("roo_mesh_smooth_test: ok\n");
    return 0;
}
