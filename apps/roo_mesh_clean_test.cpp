// roo_mesh_clean_test.cpp -- roo::MeshComponents, roo::MeshFilter and the min_faces / largest forms of roo::SaveMeshIndexed from C++
// (include/kangaroo/MarchingCubes.h over include/kfx_mesh_clean.h) on the three-sphere volume: 48^3 cells in [-1, 1]^3, the minimum of
// three sphere distances -- two spheres of 2556 and 2260 faces and a floater of 132 beside them.
//   * MeshComponents of the indexed mesh: 3 components, numbered by their smallest vertex, each closed (V = T/2 + 2), checked against
//     a union-find over the downloaded faces on the host;
//   * MeshFilter / SaveMeshIndexed(min_faces = 1000): T' = 4816, V' = 2412, the rows of the kept vertices bit for bit and in order, the
//     faces renumbered; largest: T' = 2556; min_faces = 0: the input bit for bit;
//   * SlabVolume::SaveMeshIndexed with a filter is refused, and says why.
// Prints "roo_mesh_clean_test: ok" and exits 0 when every check holds.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include <unistd.h>

#include <kangaroo/kangaroo.h>
#include <kangaroo/SlabVolume.h>

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

// the host's answer: smallest vertex id of every vertex's component (union by smaller root, then a flatten)
static std::vector<uint32_t> SmallestIds(const std::vector<uint32_t>& faces, size_t nvert)
{
    std::vector<uint32_t> parent(nvert);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) { while (parent[x] != x) x = parent[x] = parent[parent[x]]; return x; };
    for (size_t f = 0; f < faces.size() / 3; ++f)
        for (int k = 0; k < 2; ++k) {
            const uint32_t a = find(faces[3 * f + k]), b = find(faces[3 * f + k + 1]);
            if (a != b) parent[std::max(a, b)] = std::min(a, b);
        }
    for (uint32_t v = 0; v < nvert; ++v) parent[v] = find(v);
    return parent;
}

// a device copy of host words
static mesh_detail::DeviceBuffer Upload(const void* host, size_t bytes)
{
    mesh_detail::DeviceBuffer d(bytes);
    if (bytes) GpuCheckStatus(kfx_memcpy_2d(d.get(), bytes, host, bytes, bytes, 1, 1, 0));
    return d;
}

// what the filter must return for the components `keep` says to keep: rows in order, bit for bit; faces renumbered
static bool IsSelection(const mesh_detail::HostMesh& got, const mesh_detail::HostMesh& in, const std::vector<uint32_t>& vc, const std::vector<char>& keep)
{
    std::vector<uint32_t> remap(in.nvert, 0xffffffffu);
    size_t nv = 0, nt = 0;
    for (size_t v = 0; v < in.nvert; ++v)
        if (keep[vc[v]]) {
            if (nv >= got.nvert || memcmp(&got.v[3 * nv], &in.v[3 * v], 12) || memcmp(&got.n[3 * nv], &in.n[3 * v], 12)) return false;
            remap[v] = (uint32_t)nv++;
        }
    for (size_t t = 0; t < in.ntri; ++t)
        if (keep[vc[in.faces[3 * t]]]) {
            for (int k = 0; k < 3; ++k)
                if (nt >= got.ntri || got.faces[3 * nt + k] != remap[in.faces[3 * t + k]]) return false;
            ++nt;
        }
    return nv == got.nvert && nt == got.ntri && got.v.size() == 3 * nv && got.n.size() == 3 * nv && got.faces.size() == 3 * nt;
}

int main()
{
    if (kfx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    const std::string tmp = "/tmp/roo_mesh_clean_test." + std::to_string((long)getpid());
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
    const mesh_detail::DeviceBuffer dv = Upload(m.v.data(), m.v.size() * 4), dn = Upload(m.n.data(), m.n.size() * 4), df = Upload(m.faces.data(), m.faces.size() * 4);

    // ---- MeshComponents ----
    std::vector<uint32_t> vc, cf;
    const size_t C = MeshComponents(df.get<uint32_t>(), m.ntri, m.nvert, vc, cf);
    CHECK(C == 3 && vc.size() == m.nvert && cf.size() == 3);
    const std::vector<uint32_t> least = SmallestIds(m.faces, m.nvert);
    std::vector<uint32_t> roots, want_cf(C, 0), verts_of(C, 0);
    for (uint32_t v = 0; v < m.nvert; ++v)
        if (least[v] == v) roots.push_back(v);
    CHECK(roots.size() == C);
    bool labels = roots.size() == C;
    for (uint32_t v = 0; labels && v < m.nvert; ++v) {
        labels = vc[v] < C && roots[vc[v]] == least[v];   // numbered in ascending order of their smallest vertex
        if (labels) ++verts_of[vc[v]];
    }
    CHECK(labels);
    for (size_t t = 0; labels && t < m.ntri; ++t) ++want_cf[vc[m.faces[3 * t]]];
    CHECK(cf == want_cf);
    std::vector<uint32_t> sorted = cf;
    std::sort(sorted.begin(), sorted.end());
    CHECK(sorted == (std::vector<uint32_t>{132, 2260, 2556}));
    for (size_t c = 0; c < C && c < cf.size(); ++c) CHECK(verts_of[c] == cf[c] / 2 + 2);   // each part closed

    // ---- MeshFilter ----
    {
        std::vector<char> keep(C);
        for (size_t c = 0; c < C; ++c) keep[c] = cf[c] >= 1000;
        const mesh_detail::HostMesh big = MeshFilter(dv.get<float>(), dn.get<float>(), nullptr, df.get<uint32_t>(), m.nvert, m.ntri, 1000, false);
        CHECK(big.ntri == 4816 && big.nvert == 2412 && !big.color && IsSelection(big, m, vc, keep));
        for (size_t c = 0; c < C; ++c) keep[c] = cf[c] == 2556;
        const mesh_detail::HostMesh one = MeshFilter(dv.get<float>(), dn.get<float>(), nullptr, df.get<uint32_t>(), m.nvert, m.ntri, 0, true);
        CHECK(one.ntri == 2556 && one.nvert == 2556 / 2 + 2 && IsSelection(one, m, vc, keep));
        const mesh_detail::HostMesh same = MeshFilter(dv.get<float>(), dn.get<float>(), nullptr, df.get<uint32_t>(), m.nvert, m.ntri, 0, false);
        CHECK(same.nvert == m.nvert && same.ntri == m.ntri && same.faces == m.faces && !memcmp(same.v.data(), m.v.data(), m.v.size() * 4) &&
              !memcmp(same.n.data(), m.n.data(), m.n.size() * 4));
        const mesh_detail::HostMesh none = MeshFilter(dv.get<float>(), nullptr, nullptr, df.get<uint32_t>(), m.nvert, m.ntri, 2557, true);
        CHECK(none.nvert == 0 && none.ntri == 0 && none.v.empty() && none.faces.empty());
    }

    // ---- SaveMeshIndexed(min_faces, largest): the filtered arrays in the file ----
    {
        size_t nvert = 0;
        CHECK(SaveMeshIndexed(tmp, vol, 1000, false, &nvert) == 4816 && nvert == 2412);
        const mesh_detail::HostMesh want = mesh_detail::Extract(vol.abi(), KFX_CELL_F32, nullptr, 0, 0, nullptr, true, mesh_detail::MeshKeep{1000, false});
        std::vector<unsigned char> b;
        if (FILE* f = fopen((tmp + ".ply").c_str(), "rb")) {
            unsigned char buf[1 << 16];
            size_t n;
            while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
            fclose(f);
        }
        const char* end = "end_header\n";
        const auto it = std::search(b.begin(), b.end(), end, end + strlen(end));
        CHECK(it != b.end());
        const size_t body = (size_t)(it - b.begin()) + strlen(end);
        CHECK(want.nvert == 2412 && want.ntri == 4816 && b.size() == body + 24 * want.nvert + 13 * want.ntri);
        bool rows = b.size() == body + 24 * want.nvert + 13 * want.ntri;
        for (size_t v = 0; rows && v < want.nvert; ++v)
            rows = !memcmp(&b[body + 24 * v], &want.v[3 * v], 12) && !memcmp(&b[body + 24 * v + 12], &want.n[3 * v], 12);
        for (size_t t = 0; rows && t < want.ntri; ++t) rows = b[body + 24 * want.nvert + 13 * t] == 3 && !memcmp(&b[body + 24 * want.nvert + 13 * t + 1], &want.faces[3 * t], 12);
        CHECK(rows);
        CHECK(SaveMeshIndexed(tmp, vol, 0, true, &nvert) == 2556 && nvert == 2556 / 2 + 2);
        CHECK(SaveMeshIndexed(tmp, vol, 0, false, &nvert) == 4948 && nvert == 2480);
        CHECK(SaveMeshIndexed(tmp, vol, &nvert) == 4948 && nvert == 2480);
        remove((tmp + ".ply").c_str());
    }

    // ---- a slab's mesh is welded within its rank: the filter is refused there ----
    {
        kfx_comm comm;
        GpuCheckStatus(kfx_comm_create_threads(&comm, 1));
        {
            SlabVolume slab(N, N, N, bb, &comm);
            bool refused = false;
            try {
                slab.SaveMeshIndexed(tmp + ".slab", 1000, false);
            } catch (const std::invalid_argument& e) {
                refused = strstr(e.what(), "slab boundaries") != nullptr;
            }
            CHECK(refused);
            CHECK(access((tmp + ".slab.ply").c_str(), F_OK) != 0);
        }
        comm.destroy(&comm);
    }

    if (g_fail) {
        printf("roo_mesh_clean_test: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("roo_mesh_clean_test: ok\n");
    return 0;
}
