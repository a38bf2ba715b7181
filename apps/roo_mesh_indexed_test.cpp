// roo_mesh_indexed_test.cpp -- roo::SaveMeshIndexed and SlabVolume::SaveMeshIndexed from C++ (include/kangaroo/MarchingCubes.h,
// SlabVolume.h) against the plain calls (include/kfx_mesh_index.h) and the soup files of SaveMesh:
//   * SaveMeshIndexed(BoundedVolume<SDF_t | SDF_h>[, colour]) writes the index plan / indexed emit arrays of the volume, bit for bit;
//     de-indexed, the file is SaveMesh's file to within 4 ulp of the largest box coordinate, triangle for triangle;
//   * SlabVolume::SaveMeshIndexed of 3 ranks (planes copied from one volume): each rank's file de-indexes to that rank's SaveMesh
//     file within the same bound, with the same face count.
// Prints "passed" and exits 0 when every check holds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
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

// a binary PLY this library wrote: vertex records (6 floats, or 10 with colour) and three vertex ids per face
struct Ply {
    std::vector<float> rec;
    std::vector<uint32_t> faces;
    size_t nvert = 0, ntri = 0;
    int floats = 0;
    bool ok = false;
};
static Ply ReadPly(const std::string& path)
{
    Ply p;
    std::vector<unsigned char> b;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return p;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    const char* end = "end_header\n";
    auto it = std::search(b.begin(), b.end(), end, end + strlen(end));
    if (it == b.end()) return p;
    const std::string head(b.begin(), it);
    sscanf(strstr(head.c_str(), "element vertex"), "element vertex %zu", &p.nvert);
    sscanf(strstr(head.c_str(), "element face"), "element face %zu", &p.ntri);
    p.floats = strstr(head.c_str(), "property float alpha") ? 10 : 6;
    const size_t body = (size_t)(it - b.begin()) + strlen(end);
    if (b.size() != body + p.nvert * p.floats * 4 + p.ntri * 13) return p;   // the whole file: header, vertex records, faces
    p.rec.resize(p.nvert * p.floats);
    memcpy(p.rec.data(), b.data() + body, p.rec.size() * 4);
    p.faces.resize(p.ntri * 3);
    const unsigned char* q = b.data() + body + p.rec.size() * 4;
    for (size_t t = 0; t < p.ntri; ++t, q += 13) {
        if (q[0] != 3) return p;
        memcpy(&p.faces[t * 3], q + 1, 12);
    }
    p.ok = true;
    return p;
}

// the file holds the arrays of the plain calls
static bool HoldsArrays(const Ply& p, const mesh_detail::HostMesh& m)
{
    const int f = m.color ? 10 : 6;
    if (!p.ok || p.floats != f || p.nvert != m.nvert || p.ntri != m.ntri) return false;
    for (size_t i = 0; i < m.nvert; ++i) {
        if (memcmp(&p.rec[i * f], &m.v[i * 3], 12) || memcmp(&p.rec[i * f + 3], &m.n[i * 3], 12)) return false;
        if (m.color && memcmp(&p.rec[i * f + 6], &m.c[i * 4], 16)) return false;
    }
    return p.faces == m.faces;
}

// the indexed file de-indexes to the soup file: same faces in order, every corner's position within tol of the soup's copy; every id
// below the vertex count and every vertex used
static bool DeindexesTo(const Ply& idx, const Ply& soup, float tol)
{
    if (!idx.ok || !soup.ok || idx.ntri != soup.ntri || soup.nvert != 3 * soup.ntri || idx.floats != soup.floats) return false;
    std::vector<char> used(idx.nvert, 0);
    for (size_t k = 0; k < idx.faces.size(); ++k) {
        const uint32_t i = idx.faces[k];
        if (i >= idx.nvert || soup.faces[k] != k) return false;
        used[i] = 1;
        for (int c = 0; c < 3; ++c)
            if (!(std::fabs(idx.rec[(size_t)i * idx.floats + c] - soup.rec[k * soup.floats + c]) <= tol)) return false;
    }
    return std::find(used.begin(), used.end(), 0) == used.end();
}

template <typename T, typename M>
static void ToHost(std::vector<T>& out, const BoundedVolume<T, TargetDevice, M>& v)
{
    const size_t row = v.w * sizeof(T);
    out.resize((size_t)v.w * v.h * v.d);
    GpuCheckStatus(kfx_memcpy_2d(out.data(), row, v.ptr, v.pitch, row, (size_t)v.h * v.d, 2, 0));
}

template <typename CELL>
static void WholeVolume(const std::string& tmp, size_t W, size_t H, size_t D, const BoundingBox& bb, BoundedVolume<float, TargetDevice, Manage>& col, float tol)
{
    BoundedVolume<CELL, TargetDevice, Manage> vol(W, H, D, bb);
    SdfSphere(vol, make_float3(0.05f, -0.1f, 0.1f), 0.75f);
    const int cell = mesh_detail::Cell<CELL>::kind;
    size_t nvert = 0;
    const size_t ntri = SaveMeshIndexed(tmp + ".i", vol, &nvert);
    const mesh_detail::HostMesh m = mesh_detail::Extract(vol.abi(), cell, nullptr, 0, 0, nullptr, true);
    const Ply got = ReadPly(tmp + ".i.ply");
    CHECK(ntri == m.ntri && nvert == m.nvert && m.ntri > 2000 && m.nvert < m.ntri);   // (a soup has 3 vertices per triangle)
    CHECK(HoldsArrays(got, m));
    CHECK(SaveMesh(tmp + ".s", vol) == ntri);
    CHECK(DeindexesTo(got, ReadPly(tmp + ".s.ply"), tol));
    // with a colour volume
    const size_t ntc = SaveMeshIndexed(tmp + ".ic", vol, col, &nvert);
    const mesh_detail::HostMesh mc = mesh_detail::Extract(vol.abi(), cell, nullptr, 0, 0, col.abi(), true);
    const Ply gotc = ReadPly(tmp + ".ic.ply");
    CHECK(ntc == ntri && nvert == m.nvert && mc.color && gotc.floats == 10 && HoldsArrays(gotc, mc));
    CHECK(SaveMesh(tmp + ".sc", vol, col) == ntri);
    CHECK(DeindexesTo(gotc, ReadPly(tmp + ".sc.ply"), tol));
    for (const char* s : {".i.ply", ".s.ply", ".ic.ply", ".sc.ply"}) remove((tmp + s).c_str());
}

int main()
{
    if (kfx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    const std::string tmp = "/tmp/roo_mesh_indexed_test." + std::to_string((long)getpid());
    const BoundingBox bb(make_float3(-1.0f, -0.9f, -1.1f), make_float3(1.0f, 0.8f, 1.2f));
    const size_t W = 60, H = 52, D = 70;
    const float tol = 4.0f * (std::nextafter(1.2f, 2.0f) - 1.2f);   // 4 ulp of the largest |box coordinate|

    BoundedVolume<float, TargetDevice, Manage> col(W, H, D, bb);
    {
        std::vector<float> c(W * H * D);
        for (size_t i = 0; i < c.size(); ++i) c[i] = (float)((i * 2654435761u) % 1000u) / 1000.0f;
        col.MemcpyFromHost(c.data());
    }
    // ---- whole volumes, fp32 and half cells: the file against the plain calls' arrays and against SaveMesh's file ----
    WholeVolume<SDF_t>(tmp, W, H, D, bb, col, tol);
    WholeVolume<SDF_h>(tmp, W, H, D, bb, col, tol);

    // ---- SlabVolume::SaveMeshIndexed: each of 3 ranks' files de-indexes to that rank's SaveMesh file ----
    {
        BoundedVolume<SDF_t, TargetDevice, Manage> full(W, H, D, bb);
        SdfSphere(full, make_float3(0.05f, -0.1f, 0.1f), 0.75f);
        std::vector<SDF_t> hfull;
        ToHost(hfull, full);
        const size_t whole = SaveMesh(tmp + ".whole", full);
        size_t whole_verts = 0;
        CHECK(SaveMeshIndexed(tmp + ".whole", full, &whole_verts) == whole);
        remove((tmp + ".whole.ply").c_str());
        const int world = 3;
        std::vector<kfx_comm> comms(world);
        GpuCheckStatus(kfx_comm_create_threads(comms.data(), world));
        size_t sum = 0, verts = 0;
        for (int r = 0; r < world; ++r) {
            SlabVolume slab(W, H, D, bb, &comms[r]);
            slab.local.MemcpyFromHost(hfull.data() + slab.layout.s0 * W * H);
            const std::string name = tmp + ".r" + std::to_string(r);
            size_t nvert = 0;
            const size_t n = slab.SaveMeshIndexed(name + ".i", &nvert);
            CHECK(slab.SaveMesh(name + ".s") == n && n > 0);
            const Ply idx = ReadPly(name + ".i.ply");
            CHECK(idx.nvert == nvert && idx.ntri == n && nvert < 3 * n);
            CHECK(DeindexesTo(idx, ReadPly(name + ".s.ply"), tol));
            sum += n;
            verts += nvert;
            remove((name + ".i.ply").c_str()); remove((name + ".s.ply").c_str());
        }
        comms[0].destroy(&comms[0]);
        CHECK(sum == whole && whole > 2000);
        CHECK(verts > whole_verts && verts < whole_verts + 4 * W * H);   // vertices on the two slab boundaries exist once per rank
    }

    if (g_fail) {
        printf("roo_mesh_indexed_test: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("roo_mesh_indexed_test: SaveMeshIndexed and SlabVolume::SaveMeshIndexed match the plain calls and de-index to SaveMesh's files: passed\n");
    return 0;
}
