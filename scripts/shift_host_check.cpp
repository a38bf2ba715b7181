// shift_host_check.cpp -- the planner of kfx_volume_shift (kangaroo_amd/csrc/shift_host.h) under the host sanitizers, on a machine
// without a device: for a 40 x 24 x 16 volume, the shifts and the scratch sizes of tests/test_shift_plan_cpu.py (and extreme shifts
// up to INT_MAX / INT_MIN), every step of the plan is executed on host arrays that are exactly as large as the volume and the
// scratch -- so a plane index out of range is an out-of-bounds access the address sanitizer reports -- no step reads what it writes,
// and the result is the shifted volume.  Also the box arithmetic and the scratch minimum.  The kernel and the entry points' argument
// checks are not covered here (tests/test_abi_shift_cpu.py, tests/test_gpu_shift.py).
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all scripts/shift_host_check.cpp \
//       -o shift_host_check && ./shift_host_check
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../kangaroo_amd/csrc/shift_host.h"

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) { fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); abort(); } \
    } while (0)

static const int W = 40, H = 24, D = 16;
static const uint64_t FILLV = ~0ull;

// dst planes [d0, d1) = src planes [s0, s1) shifted in x and y, the fill where the source is outside
static void copy_planes(std::vector<uint64_t>& dst, int d0, int d1, const std::vector<uint64_t>& src, int s0, int sx, int sy)
{
    for (int p = 0; p < d1 - d0; ++p)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const long long xs = (long long)x + sx, ys = (long long)y + sy;
                const bool in = xs >= 0 && xs < W && ys >= 0 && ys < H;
                dst.at(((size_t)(d0 + p) * H + y) * W + x) = in ? src.at(((size_t)(s0 + p) * H + ys) * W + xs) : FILLV;
            }
}

static int run(const int s[3], size_t planes)
{
    const kfx::ShiftGeom g{W, H, D, s[0], s[1], s[2], (size_t)W * H * 8};
    std::vector<uint64_t> vol((size_t)W * H * D), scratch(planes * W * H), want(vol.size());
    for (size_t i = 0; i < vol.size(); ++i) vol[i] = i + 1;
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const long long xs = (long long)x + s[0], ys = (long long)y + s[1], zs = (long long)z + s[2];
                const bool in = xs >= 0 && xs < W && ys >= 0 && ys < H && zs >= 0 && zs < D;
                want[((size_t)z * H + y) * W + x] = in ? vol[((size_t)zs * H + ys) * W + xs] : FILLV;
            }
    const bool staged = kfx::shift_is_staged(g);
    CHECK((kfx::shift_min_scratch(g) != 0) == staged && kfx::shift_min_scratch(g) % 256 == 0 && kfx::shift_min_scratch(g) <= g.plane_bytes + 255);
    int seen = 0;
    const int n = kfx::shift_plan(g, planes, [&](const kfx_shift_step& st) {
        ++seen;
        CHECK(st.dst_z0 >= 0 && st.dst_z0 < st.dst_z1);
        const int np = st.dst_z1 - st.dst_z0;
        if (st.kind != KFX_SHIFT_FILL) CHECK(st.src_z0 >= 0 && st.src_z1 - st.src_z0 == np);
        switch (st.kind) {
        case KFX_SHIFT_FILL:
            CHECK(st.dst_z1 <= D);
            for (size_t i = (size_t)st.dst_z0 * W * H; i < (size_t)st.dst_z1 * W * H; ++i) vol.at(i) = FILLV;
            break;
        case KFX_SHIFT_DIRECT: {
            CHECK(st.dst_z1 <= D && st.src_z1 <= D && st.src_z0 - st.dst_z0 == s[2]);
            CHECK(st.dst_z1 <= st.src_z0 || st.src_z1 <= st.dst_z0);   // the launch reads no plane that it writes
            const std::vector<uint64_t> before = vol;                   // (workgroups run in no order: read the state before the launch)
            copy_planes(vol, st.dst_z0, st.dst_z1, before, st.src_z0, s[0], s[1]);
            break;
        }
        case KFX_SHIFT_STAGE:
            CHECK(staged && (size_t)st.dst_z1 <= planes && st.src_z1 <= D);
            copy_planes(scratch, st.dst_z0, st.dst_z1, vol, st.src_z0, 0, 0);
            break;
        case KFX_SHIFT_PLACE:
            CHECK(staged && (size_t)st.src_z1 <= planes && st.dst_z1 <= D);
            copy_planes(vol, st.dst_z0, st.dst_z1, scratch, st.src_z0, s[0], s[1]);
            break;
        default:
            CHECK(!"unknown kind");
        }
    });
    CHECK(n == seen && n <= 2 * D + 1);
    CHECK((n == 0) == kfx::shift_is_zero(g));
    CHECK(vol == want);
    return n;
}

int main()
{
    const int shifts[][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 3, 0}, {0, 0, -5}, {3, -2, 5}, {-7, 5, -1}, {39, 23, 15}, {40, 0, 0}, {0, 0, -16}, {0, 0, 0},
                             {0, 0, 1}, {0, 0, 15}, {0, 0, -15}, {-39, -23, -15}, {INT_MAX, 0, 0}, {0, INT_MIN, 0}, {0, 0, INT_MIN}, {1, 1, INT_MAX},
                             {INT_MIN, INT_MIN, INT_MIN}};
    const size_t planes[] = {1, 3, 16, 1000};
    int plans = 0, steps = 0;
    for (const auto& s : shifts)
        for (const size_t p : planes) { steps += run(s, p); ++plans; }
    // the box: VoxelPositionInUnits of the shifted first and last voxel; on a lattice of multiples of 1/16 exact
    kfx_volume v{};
    v.w = v.h = v.d = 32;
    const float lo[3] = {-1.0f, -1.0f, 2.0f}, hi[3] = {0.9375f, 0.9375f, 3.9375f};
    memcpy(v.boxmin, lo, sizeof(lo));
    memcpy(v.boxmax, hi, sizeof(hi));
    const int by[3] = {8, 0, -8};
    float bmin[3], bmax[3];
    kfx::shift_box(v, by, bmin, bmax);
    CHECK(bmin[0] == -0.5f && bmin[1] == -1.0f && bmin[2] == 1.5f && bmax[0] == 1.4375f && bmax[1] == 0.9375f && bmax[2] == 3.4375f);
    const int far[3] = {INT_MAX, INT_MIN, 0};
    kfx::shift_box(v, far, bmin, bmax);
    CHECK(bmin[0] > 1e8f && bmax[1] < -1e8f && bmin[2] == 2.0f);
    CHECK(kfx::shift_cell_bytes(KFX_CELL_F32) == 8 && kfx::shift_cell_bytes(KFX_CELL_F16) == 4 && kfx::shift_cell_bytes(KFX_CELL_COLOR) == 4 &&
          kfx::shift_cell_bytes(3) == 0 && kfx::shift_cell_bytes(-1) == 0);
    printf("shift_host_check: ok (%d plans, %d steps)\n", plans, steps);
    return 0;
}
