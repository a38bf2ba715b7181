// roo_brick_mesh_indexed_test.cpp -- roo::MeshBricksIndexPlan / MeshBricksEmitIndexed / SaveMeshBricksIndexed from C++
// (include/kangaroo/VolumeBricks.h over include/kfx_mesh_bricks_index.h): a small ragged volume with a sphere and unobserved cells
// is packed into bricks, the bricks are meshed as a soup with its cube list (roo_brick_mesh_test.cpp checks that soup), and the soup
// is welded on the host -- sequential first occurrence, keyed by lattice edge, the edges read from the case tables and the host copy
// of the volume.  Then:
//   * the wrappers' indexed mesh is that weld: vertex and normal bits, faces exactly;
//   * at least one lattice edge has another first cube in brick order than in dense order (the rule that is the bricks' own);
//   * with every other brick left out it is the weld of that soup;
//   * SaveMeshBricksIndexed writes those arrays: V vertex records of 24 bytes, T faces of 13.
// Prints "passed" and exits 0 when every check holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <unistd.h>

#include <kangaroo/kangaroo.h>
#include <kangaroo/VolumeBricks.h>

#include "../kangaroo_amd/csrc/mc_tables.inc"   // the case tables the library is compiled from (host arrays)

using namespace roo;

static int g_fail = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { ++g_fail; fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// the cube's corners and edges as the tables number them (kangaroo_amd/csrc/mesh_cube.h)
static int CornerDx(int i) { return ((i + 1) >> 1) & 1; }
static int CornerDy(int i) { return (i >> 1) & 1; }
static int CornerDz(int i) { return i >> 2; }
static int EdgeC0(int e) { return e < 8 ? e : e - 8; }
static int EdgeC1(int e) { return e < 4 ? (e + 1) & 3 : (e < 8 ? 4 + ((e + 1) & 3) : e - 4); }

struct Welded {
    std::vector<float> v, n;
    std::vector<uint32_t> faces;
    size_t other = 0;   // lattice edges whose first cube in the soup's order is not the lowest cube index among the cubes using them
};

// the weld of a brick soup with its cube list; val: the host copy of the volume the bricks unpack into
static Welded Weld(const mesh_detail::HostMesh& soup, const std::vector<long long>& ci, const std::vector<unsigned>& to, const std::vector<SDF_t>& val,
                   int w, int h, int d)
{
    Welded out;
    std::map<long long, uint32_t> id_of;
    std::map<long long, long long> lowest;
    std::vector<long long> first_cube;
    for (size_t k = 0; k < ci.size(); ++k) {
        const int z = (int)(ci[k] % (d - 1)), y = (int)((ci[k] / (d - 1)) % (h - 1)), x = (int)(ci[k] / ((long long)(d - 1) * (h - 1)));
        int flag = 0;
        for (int c = 0; c < 8; ++c) {
            const float f = val[((size_t)(z + CornerDz(c)) * h + y + CornerDy(c)) * w + x + CornerDx(c)].val;
            CHECK(std::isfinite(f));
            if (f <= 0.0f) flag |= 1 << c;
        }
        const size_t ntri = (k + 1 < to.size() ? to[k + 1] : soup.ntri) - to[k];
        CHECK(ntri == MC_NUM_TRIS[flag]);
        if (ntri != MC_NUM_TRIS[flag]) return out;
        for (size_t t = 0; t < 3 * ntri; ++t) {
            const int e = MC_TRIS[flag][t], c0 = EdgeC0(e), c1 = EdgeC1(e);
            const long long X = x + std::min(CornerDx(c0), CornerDx(c1)), Y = y + std::min(CornerDy(c0), CornerDy(c1)), Z = z + std::min(CornerDz(c0), CornerDz(c1));
            const int axis = CornerDx(c0) != CornerDx(c1) ? 0 : (CornerDy(c0) != CornerDy(c1) ? 1 : 2);
            const long long key = ((X * h + Y) * d + Z) * 3 + axis;
            const size_t s = (size_t)to[k] * 3 + t;   // the soup vertex
            auto it = id_of.find(key);
            if (it == id_of.end()) {
                it = id_of.emplace(key, (uint32_t)first_cube.size()).first;
                first_cube.push_back(ci[k]);
                lowest[key] = ci[k];
                out.v.insert(out.v.end(), &soup.v[s * 3], &soup.v[s * 3] + 3);
                out.n.insert(out.n.end(), &soup.n[s * 3], &soup.n[s * 3] + 3);
            } else {
                lowest[key] = std::min(lowest[key], ci[k]);
            }
            out.faces.push_back(it->second);
        }
    }
    for (const auto& kv : id_of) out.other += first_cube[kv.second] != lowest[kv.first];
    return out;
}

static bool IsTheWeld(const mesh_detail::HostMesh& m, const Welded& w)
{
    return m.nvert * 3 == w.v.size() && m.v.size() == w.v.size() && m.n.size() == w.n.size() && m.faces == w.faces &&
           memcmp(m.v.data(), w.v.data(), w.v.size() * 4) == 0 && memcmp(m.n.data(), w.n.data(), w.n.size() * 4) == 0;
}

// the file holds the arrays: a header that states V and T, V records of 6 floats, T faces of 13 bytes
static bool FileHolds(const std::string& path, const mesh_detail::HostMesh& m)
{
    std::vector<unsigned char> b;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    const char* end = "end_header\n";
    auto it = std::search(b.begin(), b.end(), end, end + strlen(end));
    if (it == b.end()) return false;
    const std::string head(b.begin(), it);
    size_t nvert = 0, ntri = 0;
    if (!strstr(head.c_str(), "element vertex") || !strstr(head.c_str(), "element face")) return false;
    sscanf(strstr(head.c_str(), "element vertex"), "element vertex %zu", &nvert);
    sscanf(strstr(head.c_str(), "element face"), "element face %zu", &ntri);
    const size_t body = (size_t)(it - b.begin()) + strlen(end);
    if (nvert != m.nvert || ntri != m.ntri || b.size() != body + nvert * 24 + ntri * 13) return false;
    for (size_t i = 0; i < nvert; ++i)
        if (memcmp(&b[body + i * 24], &m.v[i * 3], 12) || memcmp(&b[body + i * 24 + 12], &m.n[i * 3], 12)) return false;
    const unsigned char* q = b.data() + body + nvert * 24;
    for (size_t t = 0; t < ntri; ++t, q += 13)
        if (q[0] != 3 || memcmp(q + 1, &m.faces[t * 3], 12)) return false;
    return true;
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
    std::vector<long long> ci;
    std::vector<unsigned> to;
    const mesh_detail::HostMesh soup = mesh_detail::ExtractBricks(frame, KFX_CELL_F32, ids.ptr, packed.ptr, n, nullptr, nullptr, 0, false, false, &ci, &to);
    const Welded want = Weld(soup, ci, to, cells, w, h, d);
    CHECK(soup.ntri > 1000 && want.faces.size() == 3 * soup.ntri && want.v.size() < 9 * soup.ntri);
    printf("T = %zu, V = %zu, %zu lattice edges with another first cube than in dense order\n", (size_t)soup.ntri, want.v.size() / 3, want.other);
    CHECK(want.other >= 1);

    // the three calls one by one
    {
        const size_t nbytes = MeshBricksScratchBytes(n);
        mesh_detail::DeviceBuffer plan(nbytes);
        unsigned long long totals[2] = {0, 0};
        MeshBricksPlan(frame, KFX_CELL_F32, ids.ptr, packed.ptr, n, plan.get(), nbytes, totals);
        CHECK(totals[0] == ci.size() && totals[1] == soup.ntri);
        const size_t xbytes = MeshBricksIndexScratchBytes(n, totals);
        CHECK(xbytes >= 256 + 20 * totals[0] + 4 * n);
        mesh_detail::DeviceBuffer xs(xbytes);
        const size_t V = MeshBricksIndexPlan(frame, KFX_CELL_F32, ids.ptr, packed.ptr, n, plan.get(), nbytes, totals, xs.get(), xbytes);
        CHECK(V * 3 == want.v.size());
        mesh_detail::HostMesh m;
        m.nvert = V; m.ntri = totals[1];
        m.v.resize(V * 3); m.n.resize(V * 3); m.faces.resize(3 * m.ntri);
        mesh_detail::DeviceBuffer dv(V * 12), dn(V * 12), df(m.faces.size() * 4);
        MeshBricksEmitIndexed(frame, KFX_CELL_F32, ids.ptr, packed.ptr, n, nullptr, nullptr, 0, plan.get(), nbytes, xs.get(), xbytes, totals, V,
                              dv.get<float>(), dn.get<float>(), nullptr, df.get<unsigned>());
        dv.CopyTo(m.v.data(), V * 12); dn.CopyTo(m.n.data(), V * 12); df.CopyTo(m.faces.data(), m.faces.size() * 4);
        CHECK(IsTheWeld(m, want));
    }

    // every other brick: the comparator's volume is the host copy with the cells of the bricks left out unobserved
    std::vector<unsigned> half_ids;
    std::vector<unsigned char> all(n * BrickBytes(vol)), half;
    GpuCheckStatus(kfx_memcpy_2d(all.data(), all.size(), packed.ptr, all.size(), all.size(), 1, 2, 0));
    for (size_t k = 0; k < n; k += 2) {
        half_ids.push_back(host_ids[k]);
        half.insert(half.end(), all.begin() + k * BrickBytes(vol), all.begin() + (k + 1) * BrickBytes(vol));
    }
    const size_t m2 = half_ids.size();
    GpuCheckStatus(kfx_memcpy_2d(ids.ptr, m2 * 4, half_ids.data(), m2 * 4, m2 * 4, 1, 1, 0));
    GpuCheckStatus(kfx_memcpy_2d(packed.ptr, half.size(), half.data(), half.size(), half.size(), 1, 1, 0));
    const int nbx = (w + 7) / 8, nby = (h + 7) / 8;
    for (int z = 0; z < d; ++z)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                if (!std::binary_search(half_ids.begin(), half_ids.end(), (unsigned)(((z >> 3) * nby + (y >> 3)) * nbx + (x >> 3))))
                    cells[((size_t)z * h + y) * w + x].val = NAN;
    const mesh_detail::HostMesh fewer_soup = mesh_detail::ExtractBricks(frame, KFX_CELL_F32, ids.ptr, packed.ptr, m2, nullptr, nullptr, 0, false, false, &ci, &to);
    const mesh_detail::HostMesh fewer = mesh_detail::ExtractBricks(frame, KFX_CELL_F32, ids.ptr, packed.ptr, m2, nullptr, nullptr, 0, false, true);
    CHECK(fewer.ntri > 0 && fewer.ntri < soup.ntri && fewer.ntri == fewer_soup.ntri);
    CHECK(IsTheWeld(fewer, Weld(fewer_soup, ci, to, cells, w, h, d)));

    const std::string path = "/tmp/roo_brick_mesh_indexed_test." + std::to_string((long)getpid());
    size_t nvert = 0;
    const size_t ntri = SaveMeshBricksIndexed(path, frame, KFX_CELL_F32, ids.ptr, packed.ptr, m2, &nvert);
    CHECK(ntri == fewer.ntri && nvert == fewer.nvert && nvert > 0);
    CHECK(FileHolds(path + ".ply", fewer));
    remove((path + ".ply").c_str());
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    printf("passed\n");
    return 0;
}
