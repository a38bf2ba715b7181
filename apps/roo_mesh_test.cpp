// roo_mesh_test.cpp -- roo::SaveMesh on half-cell volumes and SlabVolume::SaveMesh from C++ (include/kangaroo/MarchingCubes.h,
// SlabVolume.h) against the arrays of the plain calls (include/kfx_mesh.h):
//   * SaveMesh(BoundedVolume<SDF_h>[, colour]) writes the plan / emit arrays of the half volume, bit for bit, and the same file as
//     SaveMesh of the widened BoundedVolume<SDF_t>;
//   * SlabVolume::SaveMesh of 3 ranks (planes copied from one volume) writes, together, the whole volume's triangles once each.
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

static std::vector<unsigned char> ReadFile(const std::string& path)
{
    std::vector<unsigned char> b;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return b;
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

// the vertex records of a PLY this library wrote (floats per vertex: 6, or 10 with colour)
static std::vector<float> PlyVertices(const std::string& path, size_t* ntri, int* floats)
{
    const std::vector<unsigned char> b = ReadFile(path);
    const char* end = "end_header\n";
    auto it = std::search(b.begin(), b.end(), end, end + strlen(end));
    std::vector<float> v;
    if (it == b.end()) return v;
    const std::string head(b.begin(), it);
    size_t nv = 0;
    sscanf(strstr(head.c_str(), "element vertex"), "element vertex %zu", &nv);
    sscanf(strstr(head.c_str(), "element face"), "element face %zu", ntri);
    *floats = strstr(head.c_str(), "property float alpha") ? 10 : 6;
    v.resize(nv * *floats);
    memcpy(v.data(), &*(it + strlen(end)), v.size() * 4);
    return v;
}

// the plain calls' arrays interleaved as the PLY stores them
static std::vector<float> Interleaved(const mesh_detail::HostMesh& m)
{
    const int f = m.color ? 10 : 6;
    std::vector<float> out(3 * m.ntri * f);
    for (size_t i = 0; i < 3 * m.ntri; ++i) {
        memcpy(&out[i * f], &m.v[i * 3], 12);
        memcpy(&out[i * f + 3], &m.n[i * 3], 12);
        if (m.color) memcpy(&out[i * f + 6], &m.c[i * 4], 16);
    }
    return out;
}

template <typename T, typename M>
static void ToHost(std::vector<T>& out, const BoundedVolume<T, TargetDevice, M>& v)
{
    const size_t row = v.w * sizeof(T);
    out.resize((size_t)v.w * v.h * v.d);
    GpuCheckStatus(kfx_memcpy_2d(out.data(), row, v.ptr, v.pitch, row, (size_t)v.h * v.d, 2, 0));
}

static bool SameBits(const std::vector<float>& a, const std::vector<float>& b)
{
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * 4) == 0);
}

int main()
{
    if (kfx_device_count() < 1) {
        fprintf(stderr, "no HIP device\n");
        return 2;
    }
    const std::string tmp = "/tmp/roo_mesh_test." + std::to_string((long)getpid());
    const BoundingBox bb(make_float3(-1.0f, -0.9f, -1.1f), make_float3(1.0f, 0.8f, 1.2f));
    const size_t W = 60, H = 52, D = 70;

    // ---- half cells: SaveMesh overloads against kfx_mesh_plan / kfx_mesh_emit, and against the widened fp32 volume ----
    BoundedVolume<SDF_h, TargetDevice, Manage> vh(W, H, D, bb);
    SdfSphere(vh, make_float3(0.05f, -0.1f, 0.1f), 0.75f);
    BoundedVolume<float, TargetDevice, Manage> col(W, H, D, bb);
    {
        std::vector<float> c(W * H * D);
        for (size_t i = 0; i < c.size(); ++i) c[i] = (float)((i * 2654435761u) % 1000u) / 1000.0f;
        col.MemcpyFromHost(c.data());
    }
    size_t nt = 0;
    int nf = 0;
    {
        const size_t ntri = SaveMesh(tmp + ".h", vh);
        const mesh_detail::HostMesh m = mesh_detail::Extract(vh.abi(), KFX_CELL_F16, nullptr, 0, 0, nullptr);
        const std::vector<float> got = PlyVertices(tmp + ".h.ply", &nt, &nf);
        CHECK(ntri == m.ntri && nt == m.ntri && nf == 6 && m.ntri > 2000);
        CHECK(SameBits(got, Interleaved(m)));
        // the same volume widened exactly into SDF_t cells: the same file
        std::vector<SDF_h> hh;
        ToHost(hh, vh);
        std::vector<SDF_t> hf(W * H * D);
        for (size_t i = 0; i < hh.size(); ++i) hf[i] = SDF_t((float)hh[i], hh[i].Weight());   // operator float: exact
        BoundedVolume<SDF_t, TargetDevice, Manage> vf(W, H, D, bb);
        vf.MemcpyFromHost(hf.data());
        CHECK(SaveMesh(tmp + ".f", vf) == ntri);
        CHECK(ReadFile(tmp + ".f.ply") == ReadFile(tmp + ".h.ply"));
        // with a colour volume
        const size_t ntc = SaveMesh(tmp + ".hc", vh, col);
        const mesh_detail::HostMesh mc = mesh_detail::Extract(vh.abi(), KFX_CELL_F16, nullptr, 0, 0, col.abi());
        const std::vector<float> gotc = PlyVertices(tmp + ".hc.ply", &nt, &nf);
        CHECK(ntc == ntri && nf == 10 && mc.color && SameBits(gotc, Interleaved(mc)));
        CHECK(SaveMesh(tmp + ".fc", vf, col) == ntri && ReadFile(tmp + ".fc.ply") == ReadFile(tmp + ".hc.ply"));
        remove((tmp + ".h.ply").c_str()); remove((tmp + ".f.ply").c_str());
        remove((tmp + ".hc.ply").c_str()); remove((tmp + ".fc.ply").c_str());
    }

    // ---- SlabVolume::SaveMesh: 3 ranks' parts = the whole mesh, every triangle once ----
    {
        BoundedVolume<SDF_t, TargetDevice, Manage> full(W, H, D, bb);
        SdfSphere(full, make_float3(0.05f, -0.1f, 0.1f), 0.75f);
        std::vector<SDF_t> hfull;
        ToHost(hfull, full);
        const size_t whole = SaveMesh(tmp + ".whole", full);
        const std::vector<float> want = PlyVertices(tmp + ".whole.ply", &nt, &nf);
        const int world = 3;
        std::vector<kfx_comm> comms(world);
        GpuCheckStatus(kfx_comm_create_threads(comms.data(), world));
        std::vector<std::vector<float> > tris;   // 18 floats each
        size_t sum = 0;
        for (int r = 0; r < world; ++r) {
            SlabVolume slab(W, H, D, bb, &comms[r]);
            const kfx_slab_layout& L = slab.layout;
            slab.local.MemcpyFromHost(hfull.data() + L.s0 * W * H);
            const std::string name = tmp + ".r" + std::to_string(r);
            const size_t n = slab.SaveMesh(name);
            const std::vector<float> part = PlyVertices(name + ".ply", &nt, &nf);
            CHECK(nt == n && part.size() == n * 18);
            for (size_t t = 0; t < n; ++t) tris.emplace_back(part.begin() + t * 18, part.begin() + (t + 1) * 18);
            sum += n;
            remove((name + ".ply").c_str());
        }
        comms[0].destroy(&comms[0]);
        std::vector<std::vector<float> > wt;
        for (size_t t = 0; t < whole; ++t) wt.emplace_back(want.begin() + t * 18, want.begin() + (t + 1) * 18);
        auto bits_less = [](const std::vector<float>& a, const std::vector<float>& b) { return memcmp(a.data(), b.data(), 18 * 4) < 0; };
        std::sort(tris.begin(), tris.end(), bits_less);
        std::sort(wt.begin(), wt.end(), bits_less);
        CHECK(sum == whole && whole > 2000);
        bool same = tris.size() == wt.size();
        for (size_t t = 0; same && t < wt.size(); ++t) same = memcmp(tris[t].data(), wt[t].data(), 18 * 4) == 0;
        CHECK(same);
        remove((tmp + ".whole.ply").c_str());
    }

    if (g_fail) {
        printf("roo_mesh_test: %d check(s) failed\n", g_fail);
        return 1;
    }
    printf("roo_mesh_test: half-cell SaveMesh overloads and SlabVolume::SaveMesh match the plain calls: passed\n");
    return 0;
}
