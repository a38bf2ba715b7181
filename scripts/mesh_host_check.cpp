// mesh_host_check.cpp -- the host side of mesh.hip under the host sanitizers, on a machine without a device: the scratch carver and the
// two layouts it carves (kfx::mesh_scratch, kfx::mesh_index_scratch) over segment counts 0, 1, 511, 512, 513 and active-cube counts 0,
// 1, 255, 256, 257, 2^31 -- every sub-buffer on a 256-byte boundary, in order, disjoint, large enough, `bytes` the end of the last, from
// a null scratch (sizing) as from a real address -- the two sizes include/kfx_mesh.h quotes, and kfx::mesh_setup's slab arithmetic at
// the edges tests/test_abi_mesh_cpu.py names (ghost planes, the last rank, a slab of one plane, a slab that leaves the volume).  The
// kernels and what needs a device are not covered here (tests/test_gpu_mesh_volumes.py, tests/test_gpu_mesh_indexed.py).
//   hipcc -std=c++17 -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//       scripts/mesh_host_check.cpp -o mesh_host_check && HIP_VISIBLE_DEVICES=-1 ./mesh_host_check
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../kangaroo_amd/csrc/mesh.hip"

int kfx::set_error(int code, const char*) { return code; }
int kfx::check_launch(const char*) { return 0; }

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
    } while (0)

struct Sub { const void* at; size_t need; };   // a sub-buffer and the bytes its user indexes

// the sub-buffers of a layout carved at `scratch`: aligned, in order, disjoint, no gap of 256 bytes or more; `bytes` ends the last
static void check_layout(uintptr_t scratch, std::initializer_list<Sub> subs, size_t bytes)
{
    uintptr_t end = scratch;   // of the sub-buffers so far
    for (const Sub& s : subs) {
        const uintptr_t at = (uintptr_t)s.at;
        CHECK((at - scratch) % 256 == 0 && at >= end && at - end < 256);
        end = at + s.need;
    }
    CHECK(bytes % 256 == 0 && scratch + bytes >= end && scratch + bytes - end < 256);
}

static kfx_volume volume(size_t w, size_t h, size_t d, size_t cell_bytes)
{
    kfx_volume v{};
    v.ptr = (void*)0x7f0000000000ull;   // (never dereferenced; high enough for a slab's virtual base, z_offset planes below it)
    v.w = w; v.h = h; v.d = d;
    v.pitch = w * cell_bytes;
    v.img_pitch = v.pitch * h;
    for (int i = 0; i < 3; ++i) { v.boxmin[i] = -1.0f; v.boxmax[i] = 1.0f; }
    return v;
}

int main()
{
    int layouts = 0;
    for (const uintptr_t scratch : {(uintptr_t)0, (uintptr_t)0x7f0000000000ull}) {
        for (const long long nseg : {0LL, 1LL, 511LL, 512LL, 513LL, 134086688LL}) {   // (the last: 2048^3)
            kfx::MeshRange r{};
            r.nseg = nseg;
            r.nblk = (nseg + kfx::MESH_BLOCK - 1) / kfx::MESH_BLOCK;
            const kfx::MeshScratch s = kfx::mesh_scratch(r, (const void*)scratch);
            const size_t nb = (size_t)r.nblk;
            check_layout(scratch, {{s.totals, 4 * 8}, {s.seg, nb * kfx::MESH_BLOCK * 2}, {s.part, nb * 8}, {s.base, nb * 16}}, s.bytes);
            CHECK((uintptr_t)s.totals == scratch && s.bytes >= kfx::MESH_HEADER);
            ++layouts;
        }
        for (const unsigned long long na : {0ull, 1ull, 255ull, 256ull, 257ull, 1ull << 31}) {
            const kfx::MeshIndexScratch x = kfx::mesh_index_scratch(na, (const void*)scratch);
            CHECK(x.nblk == (long long)((na + 255) / 256));
            const size_t n = (size_t)na, nb = (size_t)x.nblk;
            check_layout(scratch, {{x.hdr, 4 * 8}, {x.cube_index, n * 8}, {x.tri_offset, n * 4}, {x.info, n * 4}, {x.vbase, n * 4},
                                   {x.part, nb * 8}, {x.base, nb * 16}}, x.bytes);
            CHECK((uintptr_t)x.hdr == scratch && x.bytes >= kfx::MESH_HEADER);
            ++layouts;
        }
    }
    // the carver on its own: sizes that are and are not multiples of 256, a count of 0
    kfx::Carver c{0x1000};
    CHECK((uintptr_t)c.take<char>(1) == 0x1000 && (uintptr_t)c.take<char>(256) == 0x1100 && (uintptr_t)c.take<double>(0) == 0x1200 &&
          (uintptr_t)c.take<unsigned short>(129) == 0x1200 && c.bytes == 0x400);

    // the sizes include/kfx_mesh.h quotes, through the entry point
    for (const int cell : {KFX_CELL_F32, KFX_CELL_F16}) {
        const size_t cb = cell == KFX_CELL_F32 ? 8 : 4;
        const kfx_volume v512 = volume(512, 512, 512, cb), v2048 = volume(2048, 2048, 2048, cb);
        CHECK(kfx_mesh_scratch_bytes(&v512, cell, nullptr, 0, 0) == 4277504);
        CHECK(kfx_mesh_scratch_bytes(&v2048, cell, nullptr, 0, 0) == 274460416);
        const unsigned long long totals[2] = {1000, 2500}, bad[2] = {3, 2};
        CHECK(kfx_mesh_index_scratch_bytes(&v512, cell, nullptr, 0, 0, totals) == 256 + 8192 + 3 * 4096 + 256 + 256);
        CHECK(kfx_mesh_index_scratch_bytes(&v512, cell, nullptr, 0, 0, bad) == 0 && kfx_mesh_index_scratch_bytes(&v512, cell, nullptr, 0, 0, nullptr) == 0);
    }

    // mesh_setup: a 60-plane volume of 40 x 30 in three ranks of 20 planes
    const int D = 60;
    kfx::MeshParams p;
    kfx::MeshRange r;
    for (int rank = 0; rank < 3; ++rank) {
        const int z0 = 20 * rank, z1 = z0 + 20;
        for (int ghost = 0; ghost <= 2; ++ghost) {
            const int s0 = z0 - ghost > 0 ? z0 - ghost : 0, s1 = z1 + ghost < D ? z1 + ghost : D;
            const kfx_volume part = volume(40, 30, (size_t)(s1 - s0), 8);
            const kfx_slab slab = {(size_t)D, (size_t)s0, -1.0f, 1.0f};
            const int e = kfx::mesh_setup(p, r, &part, KFX_CELL_F32, &slab, z0, z1);
            CHECK(e == (ghost == 2 ? 0 : KFX_E_RANGE));   // the normals' stencil needs two planes either side
            if (e) continue;
            CHECK(r.zlo == z0 && r.zhi == (z1 < D - 1 ? z1 : D - 1) && r.nsz == 1 && r.nseg == 39LL * 29 && r.nblk == 3);
            CHECK(p.cx == 39 && p.cy == 29 && p.cz == D - 1 && p.avail_lo == s0 && p.avail_hi == s1);
        }
    }
    {
        // the last rank's cubes end at plane D - 2: its stencil needs planes up to D - 1 only
        const kfx_slab slab = {(size_t)D, 38, -1.0f, 1.0f};
        const kfx_volume v22 = volume(40, 30, 22, 8), v21 = volume(40, 30, 21, 8), v20 = volume(40, 30, 20, 8), v1 = volume(40, 30, 1, 4);
        CHECK(kfx::mesh_setup(p, r, &v22, KFX_CELL_F32, &slab, 40, 60) == 0 && r.zlo == 40 && r.zhi == 59);
        CHECK(kfx::mesh_setup(p, r, &v21, KFX_CELL_F32, &slab, 40, 60) == KFX_E_RANGE);
        // own planes outside the volume are clipped; an empty range meshes nothing
        CHECK(kfx::mesh_setup(p, r, &v22, KFX_CELL_F32, &slab, -5, 1000) == KFX_E_RANGE);
        CHECK(kfx::mesh_setup(p, r, &v22, KFX_CELL_F32, &slab, 45, 45) == 0 && r.zlo == 45 && r.zhi == 45 && r.nsz == 0 && r.nseg == 0 && r.nblk == 0);
        CHECK(kfx::mesh_setup(p, r, &v22, KFX_CELL_F32, &slab, 50, 45) == 0 && r.zhi == r.zlo && r.nseg == 0);
        // a slab that leaves the full volume; a slab of one plane with no cubes of its own
        const kfx_slab out = {(size_t)D, 50, -1.0f, 1.0f}, one = {(size_t)D, 10, -1.0f, 1.0f};
        CHECK(kfx::mesh_setup(p, r, &v20, KFX_CELL_F32, &out, 50, 60) == KFX_E_SHAPE);
        CHECK(kfx::mesh_setup(p, r, &v1, KFX_CELL_F16, &one, 10, 10) == 0 && r.nseg == 0 && p.avail_lo == 10 && p.avail_hi == 11);
        CHECK(kfx_mesh_scratch_bytes(&v1, KFX_CELL_F16, &one, 10, 10) == kfx::MESH_HEADER);
        // a whole volume: every cube plane; columns of more than one segment
        const kfx_volume whole = volume(40, 30, 130, 8);
        CHECK(kfx::mesh_setup(p, r, &whole, KFX_CELL_F32, nullptr, 7, 9) == 0 && r.zlo == 0 && r.zhi == 129 && r.nsz == 3 && r.nseg == 39LL * 29 * 3);
        CHECK(kfx::mesh_setup(p, r, &whole, 2, nullptr, 0, 0) == KFX_E_RANGE && kfx::mesh_setup(p, r, nullptr, KFX_CELL_F32, nullptr, 0, 0) == KFX_E_NULL);
    }
    printf("mesh_host_check: ok (%d layouts)\n", layouts);
    return 0;
}
