// mesh_bricks_host_check.cpp -- the host side of the brick mesh (kangaroo_amd/csrc/mesh_bricks_host.h) under the host sanitizers, on a
// machine without a device: which frames are accepted and their brick grid, the carving of the scratch from the brick counts -- every
// region inside the total, none overlapping, each large enough for what the kernels index in it (a host array of exactly that size is
// written at the first and last index, so an arithmetic slip is an out-of-bounds access the address sanitizer reports), a plan's layout
// the front of its emit's -- and the refusals of the counts, a scratch and the outputs, each with its code and in its order.
// The kernels are not covered here (tests/test_gpu_brick_mesh.py), nor the entry points (tests/test_abi_brick_mesh_cpu.py).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/mesh_bricks_host_check.cpp \
//       -o mesh_bricks_host_check && ./mesh_bricks_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../kangaroo_amd/csrc/mesh_bricks_host.h"

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
    } while (0)

using namespace kfx;

static size_t r256(unsigned long long n) { return (size_t)((n + 255) / 256 * 256); }

// the header's formula
static size_t formula(unsigned long long n, unsigned long long nc)
{
    const unsigned long long nblk = (n + 255) / 256;
    return 256 + r256(108 * n) + r256(4 * n) + r256(8 * nblk) + r256(16 * nblk) + (nc ? r256(108 * n) : 0);
}

static int check_counts(unsigned long long n, unsigned long long nc, bool touch)
{
    const BrickMeshScratch s = brick_mesh_scratch(n, nc), plan = brick_mesh_scratch(n, 0);
    CHECK(s.bytes == formula(n, nc) && plan.bytes == formula(n, 0));
    CHECK(s.nblk * BRICK_MESH_BLOCK >= n && (s.nblk == 0 || (s.nblk - 1) * BRICK_MESH_BLOCK < n));
    CHECK(s.hdr == 0 && s.nbr == 256);
    for (const size_t off : {s.nbr, s.cnt, s.part, s.base, s.cnbr, s.bytes}) CHECK(off % 256 == 0);
    CHECK(s.cnt - s.nbr >= 108 * n && s.part - s.cnt >= 4 * n && s.base - s.part >= 8 * s.nblk && s.cnbr - s.base >= 16 * s.nblk);
    CHECK(s.bytes - s.cnbr >= (nc ? 108 * n : 0));
    // a plan's layout is the front of the emit's
    CHECK(plan.nbr == s.nbr && plan.cnt == s.cnt && plan.part == s.part && plan.base == s.base && plan.bytes == s.cnbr && plan.bytes <= s.bytes);
    if (touch && n) {
        std::vector<unsigned char> scratch(s.bytes);
        const unsigned long long totals[2] = {n, 5 * n};
        memcpy(&scratch.at(s.hdr), totals, 16);
        const int slot = -1;
        memcpy(&scratch.at(s.nbr), &slot, 4);
        memcpy(&scratch.at(s.nbr + 4 * ((size_t)n * BRICK_NEIGHBOURS - 1)), &slot, 4);
        CHECK(s.nbr + 4 * (size_t)n * BRICK_NEIGHBOURS <= s.cnt);
        const unsigned v = 7;
        memcpy(&scratch.at(s.cnt), &v, 4);
        memcpy(&scratch.at(s.cnt + 4 * ((size_t)n - 1)), &v, 4);
        CHECK(s.cnt + 4 * (size_t)n <= s.part);
        memcpy(&scratch.at(s.part + 8 * ((size_t)s.nblk - 1) + 4), &v, 4);
        CHECK(s.part + 8 * (size_t)s.nblk <= s.base);
        memcpy(&scratch.at(s.base + 16 * ((size_t)s.nblk - 1) + 8), totals, 8);
        CHECK(s.base + 16 * (size_t)s.nblk <= s.cnbr);
        if (nc) {
            memcpy(&scratch.at(s.cnbr), &slot, 4);
            memcpy(&scratch.at(s.cnbr + 4 * ((size_t)n * BRICK_NEIGHBOURS - 1)), &slot, 4);
            CHECK(s.cnbr + 4 * (size_t)n * BRICK_NEIGHBOURS <= s.bytes);
        }
    }
    // the scratch's refusals, in their order: null, short, misaligned
    unsigned char* const p = (unsigned char*)(((uintptr_t)1 << 20));
    CHECK(brick_mesh_check_scratch(n, nc, nullptr, s.bytes).code == KFX_E_NULL);
    CHECK(brick_mesh_check_scratch(n, nc, p, s.bytes - 1).code == KFX_E_SHAPE && brick_mesh_check_scratch(n, nc, p + 1, s.bytes - 1).code == KFX_E_SHAPE);
    for (const int off : {1, 4, 16, 128, 255}) CHECK(brick_mesh_check_scratch(n, nc, p + off, s.bytes + 256).code == KFX_E_ALIGN);
    CHECK(brick_mesh_check_scratch(n, nc, p, s.bytes).code == 0 && brick_mesh_check_scratch(n, nc, p + 256, s.bytes + 1).code == 0);
    return 1;
}

static kfx_volume frame(size_t w, size_t h, size_t d)
{
    kfx_volume f{};
    f.w = w; f.h = h; f.d = d;   // (no storage: ptr and the pitches stay null / zero)
    for (int i = 0; i < 3; ++i) { f.boxmin[i] = -1.0f; f.boxmax[i] = 1.0f; }
    return f;
}

int main()
{
    int layouts = 0;
    for (const unsigned long long n : {0ull, 1ull, 2ull, 255ull, 256ull, 257ull, 4096ull, 70000ull, 262144ull, BRICK_MAX})
        for (const unsigned long long nc : {0ull, 1ull, 300ull, BRICK_MAX}) layouts += check_counts(n, nc, n <= 70000);
    // the figures the header and the tests quote; monotone in n; nothing of the frame in it
    CHECK(brick_mesh_scratch(0, 0).bytes == 256 && brick_mesh_scratch(1, 0).bytes == 256 + 256 + 256 + 256 + 256);
    CHECK(brick_mesh_scratch(70000, 0).bytes == 7847424);
    for (unsigned long long n = 0; n < 3000; ++n) CHECK(brick_mesh_scratch(n + 1, 0).bytes >= brick_mesh_scratch(n, 0).bytes);
    CHECK(brick_check_counts(BRICK_MAX, BRICK_MAX).code == 0 && brick_check_counts(BRICK_MAX + 1, 0).code == KFX_E_RANGE &&
          brick_check_counts(0, BRICK_MAX + 1).code == KFX_E_RANGE && brick_check_counts(~0ull, 0).code == KFX_E_RANGE);

    // frames: null, the cell kind, the dimensions kfx_mesh_plan accepts, the brick limit -- in that order
    BrickGeom g{};
    const kfx_volume ok = frame(40, 24, 16), ragged = frame(44, 29, 35), huge = frame(4096, 4096, 4096);
    CHECK(brick_check_frame(nullptr, KFX_CELL_F32, g).code == KFX_E_NULL);
    CHECK(brick_check_frame(&ok, KFX_CELL_COLOR, g).code == KFX_E_RANGE && brick_check_frame(&ok, -1, g).code == KFX_E_RANGE);
    CHECK(brick_check_frame(&ok, KFX_CELL_F32, g).code == 0 && g.nbx == 5 && g.nby == 3 && g.nbz == 2 && g.nb == 30);
    CHECK(brick_check_frame(&ragged, KFX_CELL_F16, g).code == 0 && g.nbx == 6 && g.nby == 4 && g.nbz == 5 && g.w == 44 && g.h == 29 && g.d == 35);
    CHECK(brick_check_frame(&huge, KFX_CELL_F32, g).code == 0 && g.nb == 134217728ull);
    for (const size_t bad : {(size_t)0, (size_t)1, (size_t)2, (size_t)65536, ~(size_t)0}) {
        const kfx_volume a = frame(bad, 24, 16), b = frame(40, bad, 16), c = frame(40, 24, bad);
        CHECK(brick_check_frame(&a, KFX_CELL_F32, g).code == KFX_E_SHAPE && brick_check_frame(&b, KFX_CELL_F32, g).code == KFX_E_SHAPE &&
              brick_check_frame(&c, KFX_CELL_F32, g).code == KFX_E_SHAPE);
        CHECK(brick_check_frame(&a, 7, g).code == KFX_E_RANGE);   // (the kind before the dimensions)
    }
    const kfx_volume edge = frame(3, 3, 3), big = frame(65535, 65535, 65535), most = frame(65535, 65535, 24);
    CHECK(brick_check_frame(&edge, KFX_CELL_F32, g).code == 0 && g.nb == 1 && !brick_mesh_has_color(g, &edge));
    CHECK(brick_check_frame(&big, KFX_CELL_F32, g).code == KFX_E_RANGE);   // 2^39 bricks
    CHECK(brick_check_frame(&most, KFX_CELL_F32, g).code == 0 && g.nb == 201326592ull);
    // colour: asked for and IsValid()
    const kfx_volume thin = frame(40, 7, 16);
    CHECK(brick_check_frame(&thin, KFX_CELL_F32, g).code == 0 && !brick_mesh_has_color(g, &thin));
    CHECK(brick_check_frame(&ok, KFX_CELL_F32, g).code == 0 && brick_mesh_has_color(g, &ok) && !brick_mesh_has_color(g, nullptr));

    // the outputs: present, then aligned (colours may be absent)
    const char* const p = (const char*)((uintptr_t)1 << 20);
    CHECK(brick_mesh_check_outputs(p, p, p, p, nullptr).code == 0 && brick_mesh_check_outputs(p, p, p, p, p).code == 0);
    CHECK(brick_mesh_check_outputs(nullptr, p, p, p, p).code == KFX_E_NULL && brick_mesh_check_outputs(p, nullptr, p, p, p).code == KFX_E_NULL &&
          brick_mesh_check_outputs(p, p, nullptr, p, p).code == KFX_E_NULL && brick_mesh_check_outputs(p, p, p, nullptr, p).code == KFX_E_NULL);
    CHECK(brick_mesh_check_outputs(p + 4, p, p, p, p).code == KFX_E_ALIGN && brick_mesh_check_outputs(p, p + 2, p, p, p).code == KFX_E_ALIGN &&
          brick_mesh_check_outputs(p, p, p + 1, p, p).code == KFX_E_ALIGN && brick_mesh_check_outputs(p, p, p, p + 3, p).code == KFX_E_ALIGN &&
          brick_mesh_check_outputs(p, p, p, p, p + 2).code == KFX_E_ALIGN && brick_mesh_check_outputs(p + 8, p + 4, p + 4, p + 4, p + 4).code == 0);
    CHECK(BRICK_NEIGHBOURS == 27 && BRICK_MESH_BLOCK == 256);
    printf("mesh_bricks_host_check: ok (%d layouts)\n", layouts);
    return 0;
}
