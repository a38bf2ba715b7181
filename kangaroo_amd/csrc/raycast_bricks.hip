// raycast_bricks.hip -- RaycastSdf straight from packed 8 x 8 x 8 bricks (include/kfx_raycast_bricks.h): the rendering of a FRAME, a
// virtual dense volume of which only the listed bricks exist and every other cell is NaN (colour: 0.5), without that volume.  The
// result is the plain march's (raycast.hip, k_raycast_sdf) on the volume the bricks would unpack into, bit for bit, because it is that
// march: the frame's geometry is filled by the same set_geometry; the ray, the march loop, the hit epilogue, the parameter fill and the
// pixel tiling are raycast_ray.h's, shared with raycast.hip; cell_of, the lerp tree and the gradient stencil are sampling.h's, shared
// with the dense samplers.  What is written here is where a cell comes from: an accessor that goes through the brick list
// (tests/test_gpu_brick_raycast.py pins the result against kfx_raycast_sdf / _h / _color).
//
//   k_rb_fill      one lane per list entry: (id -> position) into the open-addressing table of the scratch (raycast_bricks_host.h),
//                  a 32-bit atomicCAS on the id word; ids that are no brick of the frame are not inserted.  The tables are cleared
//                  by a memset in front of it.  The same kernel writes the header record.
//   k_rb_raycast   one ray per lane, raycast.hip's pixel tiling (32 x 2 pixels per wave, 2 x 2 waves; 16 lanes per wave at <= 160 x
//                  120 pixels).  A sample looks its base cell's brick up -- nothing if it is the brick the lane touched last -- and
//                  an absent one makes the sample NaN without a cell load (lerp is a + t (b - a): one NaN cell makes it NaN).  A
//                  sample that straddles bricks looks up only the bricks it touches, eight at the most, all at once (brick_sample).
// Memory: the lists and 16 to 32 bytes of scratch per listed brick.  Nothing in proportion to the frame.  The render never writes
// the scratch.
#include <hip/hip_fp16.h>

#include "kfx_device.h"
#include "sampling.h"
#include "raycast_ray.h"
#include "raycast_bricks_host.h"

namespace kfx {
namespace rb {

// RayParams (raycast_ray.h) and the brick lists.  The geometry members are the frame's: vol.ptr and the pitches are unused.
struct BrickRayParams : RayParams {
    unsigned nbx, nby;                        // the frame's brick grid
    const unsigned char* cells;
    const unsigned char* ccells;
    BrickTableView tab, ctab;
};

// grid: one lane per entry of the longer list.  Ids at or beyond nb are no bricks of the frame.
__global__ __launch_bounds__(256) void k_rb_fill(const unsigned* __restrict__ ids, const unsigned n, unsigned* slots, const unsigned mask, const int shift,
                                                 const unsigned* __restrict__ cids, const unsigned n_color, unsigned* cslots, const unsigned cmask,
                                                 const int cshift, const unsigned nb, unsigned* hdr, const unsigned long long cap,
                                                 const unsigned long long ccap)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const auto cas = [](unsigned* word, unsigned expected, unsigned desired) { return atomicCAS(word, expected, desired); };
    if (t < n) {
        const unsigned id = ids[t];
        if (id < nb) brick_table_insert(slots, mask, shift, id, (unsigned)t, cas);
    }
    if (t < n_color) {
        const unsigned id = cids[t];
        if (id < nb) brick_table_insert(cslots, cmask, cshift, id, (unsigned)t, cas);
    }
    if (t == 0) {
        hdr[0] = n;
        hdr[1] = n_color;
        reinterpret_cast<unsigned long long*>(hdr)[1] = cap;
        reinterpret_cast<unsigned long long*>(hdr)[2] = ccap;
    }
}

// ---- the accessor ----
// One list through its table, and the brick the lane touched last: a cell in the same brick probes nothing.
struct BrickLookup {
    BrickTableView tab;
    unsigned nbx, nby;
    unsigned last_id;
    int last_pos;
    __device__ __forceinline__ BrickLookup(const BrickTableView& t, unsigned nbx_, unsigned nby_) : tab(t), nbx(nbx_), nby(nby_), last_id(BRICK_SLOT_EMPTY), last_pos(-1) {}
    __device__ __forceinline__ unsigned id_of(int bx, int by, int bz) const { return ((unsigned)bz * nby + (unsigned)by) * nbx + (unsigned)bx; }
    __device__ __forceinline__ int find(unsigned id)
    {
        if (id != last_id) {
            last_pos = brick_table_find(tab, id);
            last_id = id;
        }
        return last_pos;
    }
};

// cell (x, y, z) of the frame, one at a time (the hit epilogue's stencils): `absent` where its brick is not listed
template <typename CELL>
struct BrickCell {
    BrickLookup& look;
    const unsigned char* cells;
    float absent;
    __device__ __forceinline__ float operator()(int x, int y, int z) const
    {
        const int s = look.find(look.id_of(x >> 3, y >> 3, z >> 3));
        if (s < 0) return absent;
        return CELL::val(cells + (size_t)s * (BRICK_CELLS * CELL::BYTES), (((z & 7) << 3) | (y & 7)) << 3 | (x & 7));
    }
};
struct ConstCell {
    float value;
    __device__ __forceinline__ float operator()(int, int, int) const { return value; }
};

// trilinear_at<>: the eight cells of a sample and their blend, on one path for every sample.  The bricks of the eight cells are S[j],
// j = dx | dy << 1 | dz << 2: along an axis the sample does not cross a brick face on -- seven cells in eight per axis -- S[j] is the
// brick without that bit, so a sample inside one brick, about (7/8)^3 of them, has S[j] = S[0] throughout.  The first probes of all
// bricks it has to look up -- the base cell's, unless it is the brick the lane touched last, and one per crossing, seven at the most
// -- are requested together, then the eight cells: two rounds of memory at the most, whatever the number of bricks, and one where
// the brick is the last one's and nothing is crossed.  An absent base brick makes the sample NaN without a cell load.
// (Measured against a variant that gave the one-brick samples the dense march's four 16-byte row-pair loads and sent only the
// straddling ones here: nearly every wave has a lane of either kind, runs both paths one after the other, and was 1.4 times slower --
// 0.49 against 0.355 ms per view, profiles/brick_raycast.)
template <typename CELL>
__device__ __forceinline__ float brick_sample(const BrickRayParams& p, BrickLookup& look, const CellPos& c)
{
    const int lx = c.ix & 7, ly = c.iy & 7, lz = c.iz & 7;
    const unsigned id0 = look.id_of(c.ix >> 3, c.iy >> 3, c.iz >> 3);
    constexpr unsigned BYTES = BRICK_CELLS * CELL::BYTES;
    const bool ox = lx == 7, oy = ly == 7, oz = lz == 7;
    const float nan = __builtin_nanf("");
    int S[8];
    unsigned key[8], pos[8];
    bool need[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        need[j] = j == 0 ? id0 != look.last_id : ((!(j & 1) || ox) && (!(j & 2) || oy) && (!(j & 4) || oz));
        const unsigned id = id0 + ((j & 1) ? 1u : 0u) + ((j & 2) ? p.nbx : 0u) + ((j & 4) ? p.nbx * p.nby : 0u);
        key[j] = pos[j] = 0u;
        if (need[j]) {
            const unsigned s = brick_slot_of(id, p.tab.shift);
            key[j] = p.tab.slots[2 * (size_t)s];
            pos[j] = p.tab.slots[2 * (size_t)s + 1];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const unsigned id = id0 + ((j & 1) ? 1u : 0u) + ((j & 2) ? p.nbx : 0u) + ((j & 4) ? p.nbx * p.nby : 0u);
        if (need[j])   // the first probe answers unless another id sits in the slot: then the whole search (rare: the table is half empty)
            S[j] = key[j] == id ? (pos[j] < p.tab.n ? (int)pos[j] : -1) : (key[j] == BRICK_SLOT_EMPTY ? -1 : brick_table_find(p.tab, id));
        else if (j == 0)
            S[0] = look.last_pos;
        else
            S[j] = ((j & 1) && !ox) ? S[j & ~1] : (((j & 2) && !oy) ? S[j & ~2] : ((j & 4) ? S[j & ~4] : -1));
    }
    look.last_id = id0;
    look.last_pos = S[0];
    if (S[0] < 0) return nan;
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        // the cell inside its brick: a coordinate that crosses wraps to 0.  An absent brick: NaN (the load goes to the list's first
        // brick, which exists: the base cell's does)
        const unsigned x = (k & 1) ? (ox ? 0 : lx + 1) : lx, y = (k & 2) ? (oy ? 0 : ly + 1) : ly, z = (k & 4) ? (oz ? 0 : lz + 1) : lz;
        const float val = CELL::val(p.cells + (size_t)(S[k] < 0 ? 0 : S[k]) * BYTES, (int)(((z << 3) | y) << 3 | x));
        v[k] = S[k] < 0 ? nan : val;
    }
    return trilinear_blend(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], c.fx, c.fy, c.fz);
}

// one ray: KernRaycastSdf (cu_raycast.cu:34-113; colour: :119-189) for pixel (u, v) -- raycast.hip's raycast_pixel with the samples,
// the gradient's cells and the colour sample's taken from the bricks
template <typename CELL, bool COLOR>
__global__ __launch_bounds__(256) void k_rb_raycast(const BrickRayParams p, const ColorGeom cv)
{
    int u, v;
    if (!ray_lane_pixel(p, p.sparse_lanes, blockIdx.x, blockIdx.y, u, v)) return;
    if (u >= p.w || v >= p.h) return;

    const RayBox box = ray_box(p, u, v);
    BrickLookup look(p.tab, p.nbx, p.nby);
    float depth = 0.0f;
    // (no bricks: every sample is NaN, and a march of NaN samples ends without a hit)
    if (enters(box) && p.tab.n != 0)
        depth = march_plain(p, box, [&look](const BrickRayParams& q, const V3 pos_w) { return brick_sample<CELL>(q, look, cell_of(q, pos_w)); });

    const auto gradient_at = [&](const V3 pos_w) { return gradient_over(p, BrickCell<CELL>{look, p.cells, __builtin_nanf("")}, pos_w); };
    if constexpr (COLOR) {
        write_ray(p, u, v, depth, gradient_at, [&](const V3 pos_w) {
            if (p.ctab.n == 0) return trilinear_over(cv, ConstCell{0.5f}, pos_w);   // (no colour bricks at all: every cell reads 0.5)
            BrickLookup clook(p.ctab, p.nbx, p.nby);
            return trilinear_over(cv, BrickCell<RayC32>{clook, p.ccells, 0.5f}, pos_w);
        });
    } else {
        write_ray(p, u, v, depth, gradient_at, PhongShade{});
    }
}

// the frame's geometry as ray_params fills a dense volume's (no storage behind it: ptr and pitches are not the frame's)
template <typename GEOM>
void rb_frame_geometry(GEOM& g, const kfx_volume* frame)
{
    kfx_volume f = *frame;
    f.ptr = nullptr;
    f.pitch = f.img_pitch = 0;
    set_geometry(g, &f);
}

} // namespace rb
} // namespace kfx

using namespace kfx;
using namespace kfx::rb;

extern "C" size_t kfx_raycast_bricks_scratch_bytes(unsigned long long n, unsigned long long n_color)
{
    if (brick_check_counts(n, n_color).code) return 0;
    return brick_ray_scratch(n, n_color).bytes;
}

extern "C" int kfx_raycast_bricks_plan(const kfx_volume* frame, const unsigned* ids, unsigned long long n, const unsigned* color_ids,
                                       unsigned long long n_color, void* scratch, size_t scratch_bytes, kfx_stream stream)
{
    const char* const what = "kfx_raycast_bricks_plan";
    BrickGeom geom;
    if (int e = refuse(brick_check_frame(frame, geom), what)) return e;
    if (int e = refuse(brick_check_counts(n, n_color), what)) return e;
    if (int e = refuse(brick_ray_check_ids(ids, n), what)) return e;
    if (int e = refuse(brick_ray_check_ids(color_ids, n_color), what)) return e;
    if (int e = refuse(brick_ray_check_scratch(n, n_color, scratch, scratch_bytes), what)) return e;
    const BrickRayScratch lay = brick_ray_scratch(n, n_color);
    unsigned char* const s = (unsigned char*)scratch;
    const hipStream_t st = (hipStream_t)stream;
    // every slot empty (id word 0xffffffff; the position word with it), then the entries
    if (lay.bytes > lay.tab)
        if (int e = hip_status(hipMemsetAsync(s + lay.tab, 0xff, lay.bytes - lay.tab, st), what)) return e;
    const unsigned long long lanes = n > n_color ? n : n_color;
    const BrickTableView t = brick_table_view(s + lay.tab, lay.t, n), ct = brick_table_view(s + lay.ctab, lay.ct, n_color);
    hipLaunchKernelGGL(k_rb_fill, dim3((unsigned)(lanes ? (lanes + 255) / 256 : 1)), dim3(256), 0, st, ids, (unsigned)n, (unsigned*)(s + lay.tab), t.mask, t.shift,
                       color_ids, (unsigned)n_color, (unsigned*)(s + lay.ctab), ct.mask, ct.shift, (unsigned)geom.nb, (unsigned*)(s + lay.hdr), lay.t.cap,
                       lay.ct.cap);
    return check_launch(what);
}

extern "C" int kfx_raycast_bricks(const kfx_image* depth, const kfx_image* norm, const kfx_image* img, const kfx_volume* frame, int cell,
                                  const unsigned* ids, const void* cells, unsigned long long n, const unsigned* color_ids, const void* color_cells,
                                  unsigned long long n_color, int color, const void* scratch, size_t scratch_bytes, const float T_wc[12],
                                  const float K[4], float near, float far, float trunc_dist, int subpix, kfx_stream stream)
{
    const char* const what = "kfx_raycast_bricks";
    if (!T_wc || !K) return set_error(KFX_E_NULL, "kfx_raycast_bricks: null argument");
    if (int e = check_render_images(depth, norm, img, img, what)) return e;
    BrickGeom geom;
    if (int e = refuse(brick_check_frame(frame, cell, geom), what)) return e;
    if (color && cell != KFX_CELL_F32) return fail_rule(what, KFX_E_RANGE, "the colour rendering takes fp32 SDF cells (as kfx_raycast_sdf_color)");
    if (int e = refuse(brick_check_counts(n, n_color), what)) return e;
    if (int e = refuse(brick_check_lists(ids, cells, n), what)) return e;
    if (int e = refuse(brick_check_lists(color_ids, color_cells, n_color), what)) return e;
    if (int e = refuse(brick_ray_check_scratch(n, n_color, scratch, scratch_bytes), what)) return e;
    const BrickRayScratch lay = brick_ray_scratch(n, n_color);
    const unsigned char* const s = (const unsigned char*)scratch;

    BrickRayParams p;
    rb_frame_geometry(p, frame);
    set_voxel_size(p, frame);
    ray_fill(p, depth, norm, img, T_wc, K, near, far, trunc_dist, subpix);
    p.nbx = (unsigned)geom.nbx;
    p.nby = (unsigned)geom.nby;
    p.cells = (const unsigned char*)cells;
    p.ccells = (const unsigned char*)color_cells;
    p.tab = brick_table_view(s + lay.tab, lay.t, n);
    p.ctab = brick_table_view(s + lay.ctab, lay.ct, n_color);
    if (p.w == 0 || p.h == 0) return 0;

    const dim3 grid = ray_tiling(p);
    ColorGeom cv{};
    if (color) rb_frame_geometry(cv, frame);   // the colour frame: the SDF frame's dimensions and box
    const hipStream_t st = (hipStream_t)stream;
    if (color) hipLaunchKernelGGL((k_rb_raycast<RayF32, true>), grid, dim3(256), 0, st, p, cv);
    else if (cell == KFX_CELL_F32) hipLaunchKernelGGL((k_rb_raycast<RayF32, false>), grid, dim3(256), 0, st, p, cv);
    else hipLaunchKernelGGL((k_rb_raycast<RayF16, false>), grid, dim3(256), 0, st, p, cv);
    return check_launch(what);
}
