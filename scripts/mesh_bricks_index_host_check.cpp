// mesh_bricks_index_host_check.cpp -- the host side of the indexed brick mesh (kangaroo_amd/csrc/mesh_bricks_host.h, the part for
// include/kfx_mesh_bricks_index.h) under the host sanitizers, on a machine without a device: the carving of the index scratch from
// the brick count and the plan's totals -- every region inside the total, none overlapping, each aligned and large enough for what
// the kernels index in it (a host array of exactly that size is written at the first and last index, so an arithmetic slip is an
// out-of-bounds access the address sanitizer reports) -- and the refusals of the totals, the index scratch and the outputs, each
// with its code and in its order.
// The kernels are not covered here (tests/test_gpu_brick_mesh_indexed.py), nor the entry points
// (tests/test_abi_brick_mesh_indexed_cpu.py).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/mesh_bricks_index_host_check.cpp
//       -o mesh_bricks_index_host_check && ./mesh_bricks_index_host_check        (one command line)
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
static size_t formula(unsigned long long n, unsigned long long a)
{
    const unsigned long long xblk = (a + 255) / 256;
    return 256 + r256(8 * a) + 3 * r256(4 * a) + r256(4 * n) + r256(8 * xblk) + r256(16 * xblk);
}

static int check_layout(unsigned long long n, unsigned long long a, bool touch)
{
    const BrickMeshIndexScratch s = brick_mesh_index_scratch(n, a);
    CHECK(s.bytes == formula(n, a));
    CHECK(s.nblk * BRICK_MESH_IDX_BLOCK >= a && (s.nblk == 0 || (s.nblk - 1) * BRICK_MESH_IDX_BLOCK < a));
    CHECK(s.hdr == 0 && s.cube_index == 256);
    const size_t off[] = {s.hdr, s.cube_index, s.tri_offset, s.info, s.vbase, s.first, s.part, s.base, s.bytes};
    const unsigned long long need[] = {32, 8 * a, 4 * a, 4 * a, 4 * a, 4 * n, 8 * s.nblk, 16 * s.nblk};
    for (int i = 0; i < 8; ++i) {   // in order, aligned, each region large enough: none overlaps the next
        CHECK(off[i] % 256 == 0 && off[i + 1] % 256 == 0 && off[i + 1] >= off[i]);
        CHECK(off[i + 1] - off[i] >= need[i]);
    }
    if (touch && n && a) {
        std::vector<unsigned char> scratch(s.bytes);
        const unsigned long long words[4] = {3 * a, 5 * a, a, 5 * a};
        memcpy(&scratch.at(s.hdr), words, 32);
        const long long ci = -1;
        const unsigned v = 7;
        memcpy(&scratch.at(s.cube_index), &ci, 8);
        memcpy(&scratch.at(s.cube_index + 8 * ((size_t)a - 1)), &ci, 8);
        for (const size_t at : {s.tri_offset, s.info, s.vbase}) {
            memcpy(&scratch.at(at), &v, 4);
            memcpy(&scratch.at(at + 4 * ((size_t)a - 1)), &v, 4);
        }
        memcpy(&scratch.at(s.first), &v, 4);
        memcpy(&scratch.at(s.first + 4 * ((size_t)n - 1)), &v, 4);
        memcpy(&scratch.at(s.part + 8 * ((size_t)s.nblk - 1) + 4), &v, 4);
        memcpy(&scratch.at(s.base + 16 * ((size_t)s.nblk - 1) + 8), words, 8);
        CHECK(s.base + 16 * (size_t)s.nblk <= s.bytes);
    }
    // the index scratch's refusals, in their order: null, short, misaligned
    const unsigned long long totals[2] = {a, 5 * a};
    unsigned char* const p = (unsigned char*)(((uintptr_t)1 << 20));
    CHECK(brick_mesh_index_check_scratch(n, totals, nullptr, s.bytes).code == KFX_E_NULL);
    CHECK(brick_mesh_index_check_scratch(n, totals, p, s.bytes - 1).code == KFX_E_SHAPE &&
          brick_mesh_index_check_scratch(n, totals, p + 1, s.bytes - 1).code == KFX_E_SHAPE);
    for (const int o : {1, 4, 16, 128, 255}) CHECK(brick_mesh_index_check_scratch(n, totals, p + o, s.bytes + 256).code == KFX_E_ALIGN);
    CHECK(brick_mesh_index_check_scratch(n, totals, p, s.bytes).code == 0 && brick_mesh_index_check_scratch(n, totals, p + 256, s.bytes + 1).code == 0);
    return 1;
}

int main()
{
    int layouts = 0;
    for (const unsigned long long n : {0ull, 1ull, 255ull, 256ull, 257ull, 70000ull, BRICK_MAX})
        for (const unsigned long long a : {0ull, 1ull, 255ull, 256ull, 257ull, 65536ull, 300001ull, BRICK_MESH_MAX_TRIS - 1})
            layouts += check_layout(n, a, n <= 70000 && a <= 300001);
    // the figures the header and the tests quote; monotone in both arguments; the frame appears nowhere
    CHECK(brick_mesh_index_scratch(0, 0).bytes == 256 && brick_mesh_index_scratch(1, 1).bytes == 256 + 4 * 256 + 256 + 256 + 256);
    CHECK(brick_mesh_index_scratch(60, 1000).bytes == 256 + 8192 + 3 * 4096 + 256 + 256 + 256);
    for (unsigned long long k = 0; k < 3000; ++k) {
        CHECK(brick_mesh_index_scratch(k + 1, 1000).bytes >= brick_mesh_index_scratch(k, 1000).bytes);
        CHECK(brick_mesh_index_scratch(60, k + 1).bytes >= brick_mesh_index_scratch(60, k).bytes);
    }
    // about 20 bytes per active cube: within a page of 20 A + 4 n + 24 xblk + 256
    for (const unsigned long long a : {1000ull, 100000ull, 2200000ull}) {
        const size_t b = brick_mesh_index_scratch(5000, a).bytes, plain = (size_t)(20 * a + 4 * 5000 + 24 * ((a + 255) / 256) + 256);
        CHECK(b >= plain && b - plain < 8 * 256);
    }

    // the totals: null, then the range a plan can have made (cubes <= triangles < 2^32 / 3), then V <= 3 T
    const unsigned long long ok[2] = {10, 30}, more_cubes[2] = {5, 4}, many[2] = {1, BRICK_MESH_MAX_TRIS}, most[2] = {1, BRICK_MESH_MAX_TRIS - 1},
                             none[2] = {0, 0};
    CHECK(brick_mesh_check_totals(nullptr, 0).code == KFX_E_NULL);
    CHECK(brick_mesh_check_totals(ok, 0).code == 0 && brick_mesh_check_totals(ok, 90).code == 0 && brick_mesh_check_totals(ok, 91).code == KFX_E_RANGE);
    CHECK(brick_mesh_check_totals(more_cubes, 0).code == KFX_E_RANGE && brick_mesh_check_totals(many, 0).code == KFX_E_RANGE);
    CHECK(brick_mesh_check_totals(most, 3 * (BRICK_MESH_MAX_TRIS - 1)).code == 0 && 3 * (BRICK_MESH_MAX_TRIS - 1) < (1ull << 32));
    CHECK(brick_mesh_check_totals(none, 0).code == 0 && brick_mesh_check_totals(none, 1).code == KFX_E_RANGE);

    // the outputs: present, then aligned (colours may be absent)
    const char* const p = (const char*)((uintptr_t)1 << 20);
    CHECK(brick_mesh_check_indexed_outputs(p, p, nullptr, p).code == 0 && brick_mesh_check_indexed_outputs(p, p, p, p).code == 0);
    CHECK(brick_mesh_check_indexed_outputs(nullptr, p, p, p).code == KFX_E_NULL && brick_mesh_check_indexed_outputs(p, nullptr, p, p).code == KFX_E_NULL &&
          brick_mesh_check_indexed_outputs(p, p, p, nullptr).code == KFX_E_NULL);
    CHECK(brick_mesh_check_indexed_outputs(p + 1, p, p, p).code == KFX_E_ALIGN && brick_mesh_check_indexed_outputs(p, p + 2, p, p).code == KFX_E_ALIGN &&
          brick_mesh_check_indexed_outputs(p, p, p + 3, p).code == KFX_E_ALIGN && brick_mesh_check_indexed_outputs(p, p, p, p + 2).code == KFX_E_ALIGN &&
          brick_mesh_check_indexed_outputs(p + 4, p + 4, p + 4, p + 4).code == 0);
    CHECK(BRICK_MESH_IDX_BLOCK == 256 && BRICK_MESH_MAX_TRIS == 1431655765ull);
    printf("mesh_bricks_index_host_check: ok (%d layouts)\n", layouts);
    return 0;
}
