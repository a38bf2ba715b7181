// bricks_host_check.cpp -- the host side of the sparse brick snapshots (kangaroo_amd/csrc/bricks_host.h) under the host sanitizers, on
// a machine without a device: the brick grid of a view, the carving of the scratch -- every region inside the total, none overlapping,
// each large enough for what the kernels index in it (a host array of exactly that size is written at the first and last index, so an
// arithmetic slip is an out-of-bounds access the address sanitizer reports) -- and the refusals of a scratch and of the lists, each
// with its code and in its order.  Dimensions run up to 65535 and beyond the brick limit, where a narrower integer would wrap.
// The kernels and the entry points' volume checks are not covered here (tests/test_abi_bricks_cpu.py, tests/test_gpu_bricks.py).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/bricks_host_check.cpp \
//       -o bricks_host_check && ./bricks_host_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../kangaroo_amd/csrc/bricks_host.h"

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
    } while (0)

using namespace kfx;

static size_t r256(unsigned long long n) { return (size_t)((n + 255) / 256 * 256); }

static int check_dims(size_t w, size_t h, size_t d, bool touch)
{
    const BrickGeom g = brick_geom(w, h, d);
    CHECK(g.w == (int)w && g.h == (int)h && g.d == (int)d);
    CHECK((size_t)g.nbx * 8 >= w && (size_t)(g.nbx - 1) * 8 < w && (size_t)g.nby * 8 >= h && (size_t)(g.nby - 1) * 8 < h &&
          (size_t)g.nbz * 8 >= d && (size_t)(g.nbz - 1) * 8 < d);
    CHECK(g.nb == (unsigned long long)g.nbx * g.nby * g.nbz);
    CHECK(g.nblk * BRICK_SCAN_BLOCK >= g.nb && (g.nblk - 1) * BRICK_SCAN_BLOCK < g.nb);
    const BrickRefusal grid = brick_check_grid(g);
    CHECK((grid.code == 0) == (g.nb <= BRICK_MAX) && (grid.code == 0 || (grid.code == KFX_E_RANGE && grid.rule)));
    const BrickScratch s = brick_scratch(g);
    // the header's formula, and the regions in order, aligned, each as large as its kernel's last index needs
    CHECK(s.bytes == 256 + r256(g.nb) + 2 * r256(4 * g.nblk));
    CHECK(s.hdr == 0 && s.flags == 256 && s.flags % 256 == 0 && s.part % 256 == 0 && s.base % 256 == 0 && s.bytes % 256 == 0);
    CHECK(s.flags - s.hdr >= 8 && s.part - s.flags >= g.nb && s.base - s.part >= 4 * g.nblk && s.bytes - s.base >= 4 * g.nblk);
    if (touch && grid.code == 0) {
        std::vector<unsigned char> scratch(s.bytes);
        unsigned long long total = g.nb;
        memcpy(&scratch.at(s.hdr), &total, 8);
        scratch.at(s.flags) = 1;
        scratch.at(s.flags + (size_t)g.nb - 1) = 1;
        unsigned v = 7;
        memcpy(&scratch.at(s.part), &v, 4);
        memcpy(&scratch.at(s.part + 4 * ((size_t)g.nblk - 1)), &v, 4);
        CHECK(s.part + 4 * ((size_t)g.nblk - 1) + 4 <= s.base);
        memcpy(&scratch.at(s.base), &v, 4);
        memcpy(&scratch.at(s.base + 4 * ((size_t)g.nblk - 1)), &v, 4);
        CHECK(s.base + 4 * ((size_t)g.nblk - 1) + 4 <= s.bytes);
        // the scratch's refusals, in their order: null, short, misaligned
        unsigned char* const p = (unsigned char*)(((uintptr_t)1 << 20));
        CHECK(brick_check_scratch(g, nullptr, s.bytes).code == KFX_E_NULL);
        CHECK(brick_check_scratch(g, nullptr, 0).code == KFX_E_NULL);
        CHECK(brick_check_scratch(g, p, s.bytes - 1).code == KFX_E_SHAPE && brick_check_scratch(g, p, 0).code == KFX_E_SHAPE);
        CHECK(brick_check_scratch(g, p + 1, s.bytes - 1).code == KFX_E_SHAPE);   // short before misaligned
        for (const int off : {1, 4, 16, 128, 255}) CHECK(brick_check_scratch(g, p + off, s.bytes + 256).code == KFX_E_ALIGN);
        CHECK(brick_check_scratch(g, p, s.bytes).code == 0 && brick_check_scratch(g, p + 256, s.bytes + 1).code == 0);
    }
    return 1;
}

int main()
{
    int n = 0;
    const size_t dims[] = {1, 7, 8, 9, 16, 40, 41, 255, 256, 257, 512, 2047, 2048, 65535};
    for (const size_t w : dims)
        for (const size_t h : dims)
            for (const size_t d : dims) n += check_dims(w, h, d, (w + 7) / 8 * ((h + 7) / 8) * ((d + 7) / 8) <= (1u << 22));
    {   // the figures the header and the tests quote
        const BrickGeom g = brick_geom(512, 512, 512);
        CHECK(g.nb == 262144 && g.nblk == 1024 && brick_scratch(g).bytes == 270592);
        const BrickGeom e = brick_geom(40, 24, 16);
        CHECK(e.nbx == 5 && e.nby == 3 && e.nbz == 2 && e.nb == 30 && e.nblk == 1 && brick_scratch(e).bytes == 256 + 256 + 512);
        const BrickGeom big = brick_geom(65535, 65535, 65535);
        CHECK(big.nb == 8192ull * 8192ull * 8192ull && brick_check_grid(big).code == KFX_E_RANGE);
        const BrickGeom edge = brick_geom(65535, 65535, 24);   // 8192 * 8192 * 3 bricks: inside the limit
        CHECK(edge.nb == 201326592ull && brick_check_grid(edge).code == 0);
    }
    {   // the lists: nothing asked of an empty one; then the count, the pointers, their alignment -- in that order
        const void* const p = (const void*)((uintptr_t)1 << 20);
        const void* const p2 = (const void*)(((uintptr_t)1 << 20) + 2), * const p8 = (const void*)(((uintptr_t)1 << 20) + 8);
        CHECK(brick_check_lists(nullptr, nullptr, 0).code == 0 && brick_check_lists(p2, p8, 0).code == 0);
        CHECK(brick_check_lists(nullptr, p, 1).code == KFX_E_NULL && brick_check_lists(p, nullptr, 1).code == KFX_E_NULL);
        CHECK(brick_check_lists(p2, p, 1).code == KFX_E_ALIGN && brick_check_lists(p, p8, 1).code == KFX_E_ALIGN);
        CHECK(brick_check_lists(p8, p, 1).code == 0 && brick_check_lists(p, p, BRICK_MAX).code == 0);
        CHECK(brick_check_lists(p, p, BRICK_MAX + 1).code == KFX_E_RANGE && brick_check_lists(nullptr, nullptr, ~0ull).code == KFX_E_RANGE);
    }
    CHECK(BRICK == 8 && BRICK_CELLS == 512 && shift_cell_bytes(KFX_CELL_F32) * BRICK_CELLS == 4096 && shift_cell_bytes(KFX_CELL_COLOR) * BRICK_CELLS == 2048);
    printf("bricks_host_check: ok (%d grids)\n", n);
    return 0;
}
