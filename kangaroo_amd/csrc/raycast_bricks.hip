// raycast_bricks.hip -- RaycastSdf straight from packed 8 x 8 x 8 bricks (include/kfx_raycast_bricks.h): the rendering of a FRAME, a
// virtual dense volume of which only the listed bricks exist and every other cell is NaN (colour: 0.5), without that volume.  The
// result is the plain march's (raycast.hip, k_raycast_sdf) on the volume the bricks would unpack into, bit for bit: the frame's
// geometry is filled by the same set_geometry, cell_of / lerp / march_step and the cell readers are sampling.h's, and the ray, the
// march, the gradient stencil, the shade and the stores below restate raycast.hip's ray_box / raycast_pixel / write_ray and
// sampling.h's gradient<> / trilinear_at<> expression for expression over an accessor that goes through the brick list
// (tests/test_gpu_brick_raycast.py pins the restatement against kfx_raycast_sdf / _h / _color).
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
#include "raycast_bricks_host.h"

namespace kfx {
namespace rb {

// RayParams' members (raycast.hip) and the brick lists.  The geometry members are the frame's: vol.ptr and the pitches are unused.
struct BrickRayParams {
    VolView vol;
    V3 size, dims1, hi2, voxel, inv_size;
    int fastdiv, off32;
    Pose T;           // T_wc
    Intr K;
    unsigned char *dptr, *nptr, *iptr;
    size_t dpitch, npitch, ipitch;
    int w, h;
    float near, far, trunc;
    int subpix;
    int tile_log2w, wg_log2x, sparse_lanes;   // raycast.hip's pixel mapping
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

// ---- raycast.hip's ray, restated ----
// PhongShade (cu_raycast.cu:14-28)
__device__ __forceinline__ float rb_phong(const V3 p_c, const V3 n_c)
{
    const float ambient = (float)0.4, diffuse = (float)0.4, specular = (float)0.2;
    const V3 eyedir = div_s(p_c * -1.0f, length(p_c));
    const V3 l0 = v3((float)0.4, (float)0.4, -1.0f);
    const V3 lightdir = div_s(l0, length(l0));
    const float ldotn = dot(lightdir, n_c);
    const V3 lightreflect = n_c * (2 * ldotn) + lightdir * -1.0f;
    const float edotr = fmaxf(0.0f, dot(eyedir, lightreflect));
    const float spec = edotr * edotr * edotr * edotr * edotr * edotr * edotr * edotr * edotr * edotr;
    return ambient + diffuse * ldotn + specular * spec;
}

// the pixel of a lane: ray_pixel_of / ray_lane_pixel
__device__ __forceinline__ bool rb_lane_pixel(const BrickRayParams& p, int bx, int by, int& u, int& v)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (!p.sparse_lanes) {
        const int tw = 1 << p.tile_log2w, th = 64 >> p.tile_log2w;
        const int wgx = 1 << p.wg_log2x, wgy = 4 >> p.wg_log2x;
        u = (bx * wgx + (wv & (wgx - 1))) * tw + (lane & (tw - 1));
        v = (by * wgy + (wv >> p.wg_log2x)) * th + (lane >> p.tile_log2w);
        return true;
    }
    u = (bx * 2 + (wv & 1)) * p.sparse_lanes + lane;
    v = by * 2 + (wv >> 1);
    return lane < p.sparse_lanes;
}

// the ray of pixel (u, v) and the slab test against the frame's box (cu_raycast.cu:40-51): ray_box
struct BrickRayBox { V3 c_w, ray_c, ray_w; float max_tmin, min_tmax; };
__device__ __forceinline__ BrickRayBox rb_ray_box(const BrickRayParams& p, const int u, const int v)
{
    BrickRayBox b;
    b.c_w = v3(p.T.m[3], p.T.m[7], p.T.m[11]);
    b.ray_c = v3(((float)u - p.K.u0) / p.K.fu, ((float)v - p.K.v0) / p.K.fv, 1.0f);
    b.ray_w = so3_mul(p.T, b.ray_c);
    const V3 ta = div_cw(p.vol.bmin - b.c_w, b.ray_w);
    const V3 tb = div_cw(p.vol.bmax - b.c_w, b.ray_w);
    const V3 tmin = v3(fminf(ta.x, tb.x), fminf(ta.y, tb.y), fminf(ta.z, tb.z));
    const V3 tmax = v3(fmaxf(ta.x, tb.x), fmaxf(ta.y, tb.y), fmaxf(ta.z, tb.z));
    b.max_tmin = fmaxf(fmaxf(fmaxf(tmin.x, tmin.y), tmin.z), p.near);
    b.min_tmax = fminf(fminf(fminf(tmax.x, tmax.y), tmax.z), p.far);
    return b;
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
    return lerp(lerp(lerp(v[0], v[1], c.fx), lerp(v[2], v[3], c.fx), c.fy), lerp(lerp(v[4], v[5], c.fx), lerp(v[6], v[7], c.fx), c.fy), c.fz);
}

// sampling.h's gradient<> (BoundedVolume::GetUnitsBackwardDiffDxDyDz), expression for expression, over a cell accessor: the base
// cell clamp(floor(pf), 1, dim - 2) on the frame's dimensions, the 20 cells of {-1, 0, 1}^3 with at most one coordinate -1
template <typename ACC>
__device__ __forceinline__ V3 rb_gradient(const BrickRayParams& p, const ACC& cell, const V3 pos_w)
{
    const V3 pos_v = div_cw(pos_w - p.vol.bmin, p.size);
    const V3 pf = v3(pos_v.x * p.dims1.x, pos_v.y * p.dims1.y, pos_v.z * p.dims1.z);
    const int ix = (int)fmaxf(fminf(p.hi2.x, floorf(pf.x)), 1.f);
    const int iy = (int)fmaxf(fminf(p.hi2.y, floorf(pf.y)), 1.f);
    const int iz = (int)fmaxf(fminf(p.hi2.z, floorf(pf.z)), 1.f);
    const float fx = pf.x - (float)ix, fy = pf.y - (float)iy, fz = pf.z - (float)iz;
    float c[2][2][2], mx[2][2], my[2][2], mz[2][2];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            mx[dz][dy] = cell(ix - 1, iy + dy, iz + dz);
            c[dz][dy][0] = cell(ix, iy + dy, iz + dz);
            c[dz][dy][1] = cell(ix + 1, iy + dy, iz + dz);
        }
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        my[dz][0] = cell(ix, iy - 1, iz + dz);
        my[dz][1] = cell(ix + 1, iy - 1, iz + dz);
    }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        mz[dy][0] = cell(ix, iy + dy, iz - 1);
        mz[dy][1] = cell(ix + 1, iy + dy, iz - 1);
    }
    V3 g[2][2][2];
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const float v0 = c[dz][dy][dx];
                const float bx = dx ? c[dz][dy][0] : mx[dz][dy];
                const float by = dy ? c[dz][0][dx] : my[dz][dx];
                const float bz = dz ? c[0][dy][dx] : mz[dy][dx];
                g[dz][dy][dx] = v3(v0 - bx, v0 - by, v0 - bz);
            }
    const V3 deriv = lerp(lerp(lerp(g[0][0][0], g[0][0][1], fx), lerp(g[0][1][0], g[0][1][1], fx), fy),
                          lerp(lerp(g[1][0][0], g[1][0][1], fx), lerp(g[1][1][0], g[1][1][1], fx), fy), fz);
    return div_cw(deriv, p.voxel);
}

// sampling.h's trilinear<> for the colour volume: its cell_of() and trilinear_at<>'s blend over a cell accessor
template <typename ACC>
__device__ __forceinline__ float rb_trilinear(const ColorGeom& cv, const ACC& cell, const V3 pos_w)
{
    const CellPos c = cell_of(cv, pos_w);
    const int ix = c.ix, iy = c.iy, iz = c.iz;
    const float c000 = cell(ix, iy, iz), c001 = cell(ix + 1, iy, iz), c010 = cell(ix, iy + 1, iz), c011 = cell(ix + 1, iy + 1, iz);
    const float c100 = cell(ix, iy, iz + 1), c101 = cell(ix + 1, iy, iz + 1), c110 = cell(ix, iy + 1, iz + 1), c111 = cell(ix + 1, iy + 1, iz + 1);
    return lerp(lerp(lerp(c000, c001, c.fx), lerp(c010, c011, c.fx), c.fy), lerp(lerp(c100, c101, c.fx), lerp(c110, c111, c.fx), c.fy), c.fz);
}

// one ray: raycast_pixel and write_ray (KernRaycastSdf, cu_raycast.cu:34-113; colour: :119-189) for pixel (u, v)
template <typename CELL, bool COLOR>
__global__ __launch_bounds__(256) void k_rb_raycast(const BrickRayParams p, const ColorGeom cv)
{
    int u, v;
    if (!rb_lane_pixel(p, blockIdx.x, blockIdx.y, u, v)) return;
    if (u >= p.w || v >= p.h) return;

    const BrickRayBox box = rb_ray_box(p, u, v);
    const V3 c_w = box.c_w, ray_w = box.ray_w;
    const float max_tmin = box.max_tmin, min_tmax = box.min_tmax;
    BrickLookup look(p.tab, p.nbx, p.nby);

    float depth = 0.0f;
    // (no bricks: every sample is NaN, and a march of NaN samples ends without a hit)
    if (max_tmin < min_tmax && p.tab.n != 0) {
        float lambda = max_tmin;
        float last_sdf = __builtin_nanf("");
        const float min_delta = p.voxel.x;
        float delta = 0.f;
        while (lambda < min_tmax) {
            const V3 pos_w = c_w + ray_w * lambda;
            const float sdf = brick_sample<CELL>(p, look, cell_of(p, pos_w));
            if (sdf <= 0) {
                if (last_sdf > 0) {
                    if (p.subpix) lambda = lambda + delta * sdf / (last_sdf - sdf);
                    depth = lambda;
                }
                break;
            }
            delta = march_step(sdf, min_delta, p.trunc);
            lambda += delta;
            last_sdf = sdf;
        }
    }

    float* const o_depth = reinterpret_cast<float*>(p.dptr + (size_t)v * p.dpitch) + u;
    float* const o_shade = reinterpret_cast<float*>(p.iptr + (size_t)v * p.ipitch) + u;
    float4* const o_normal = reinterpret_cast<float4*>(p.nptr + (size_t)v * p.npitch) + u;
    if (depth > 0) {
        const V3 pos_w = c_w + ray_w * depth;
        // the surface normal in the camera frame (cu_raycast.cu:92-97): the normalised gradient, (0, 0, 1) where it vanishes
        const V3 g = rb_gradient(p, BrickCell<CELL>{look, p.cells, __builtin_nanf("")}, pos_w);
        const float len = length(g);
        const V3 n_w = len > 0 ? div_s(g, len) : v3(0.f, 0.f, 1.f);
        const V3 n_c = so3_mul_inv(p.T, n_w);
        *o_depth = depth;
        if constexpr (COLOR) {
            if (p.ctab.n != 0) {
                BrickLookup clook(p.ctab, p.nbx, p.nby);
                *o_shade = rb_trilinear(cv, BrickCell<RayC32>{clook, p.ccells, 0.5f}, pos_w);
            } else {
                *o_shade = rb_trilinear(cv, ConstCell{0.5f}, pos_w);   // (no colour bricks at all: every cell reads 0.5)
            }
        } else {
            *o_shade = rb_phong(box.ray_c * depth, n_c);
        }
        *o_normal = make_float4(n_c.x, n_c.y, n_c.z, 1.0f);
    } else {
        // what a ray that hits nothing writes (cu_raycast.cu:104-108)
        *o_depth = __builtin_nanf("");
        *o_shade = 0.f;
        *o_normal = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

int rb_refuse(const BrickRefusal& r, const char* what) { return r.code ? fail_rule(what, r.code, r.rule) : 0; }

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
    if (brick_ray_check_counts(n, n_color).code) return 0;
    return brick_ray_scratch(n, n_color).bytes;
}

extern "C" int kfx_raycast_bricks_plan(const kfx_volume* frame, const unsigned* ids, unsigned long long n, const unsigned* color_ids,
                                       unsigned long long n_color, void* scratch, size_t scratch_bytes, kfx_stream stream)
{
    const char* const what = "kfx_raycast_bricks_plan";
    BrickGeom geom;
    if (int e = rb_refuse(brick_ray_check_frame(frame, geom), what)) return e;
    if (int e = rb_refuse(brick_ray_check_counts(n, n_color), what)) return e;
    if (int e = rb_refuse(brick_ray_check_ids(ids, n), what)) return e;
    if (int e = rb_refuse(brick_ray_check_ids(color_ids, n_color), what)) return e;
    if (int e = rb_refuse(brick_ray_check_scratch(n, n_color, scratch, scratch_bytes), what)) return e;
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
    if (int e = rb_refuse(brick_ray_check_frame(frame, cell, geom), what)) return e;
    if (color && cell != KFX_CELL_F32) return fail_rule(what, KFX_E_RANGE, "the colour rendering takes fp32 SDF cells (as kfx_raycast_sdf_color)");
    if (int e = rb_refuse(brick_ray_check_counts(n, n_color), what)) return e;
    if (int e = rb_refuse(brick_check_lists(ids, cells, n), what)) return e;
    if (int e = rb_refuse(brick_check_lists(color_ids, color_cells, n_color), what)) return e;
    if (int e = rb_refuse(brick_ray_check_scratch(n, n_color, scratch, scratch_bytes), what)) return e;
    const BrickRayScratch lay = brick_ray_scratch(n, n_color);
    const unsigned char* const s = (const unsigned char*)scratch;

    BrickRayParams p;
    rb_frame_geometry(p, frame);
    set_voxel_size(p, frame);
    for (int i = 0; i < 12; ++i) p.T.m[i] = T_wc[i];
    p.K = Intr{K[0], K[1], K[2], K[3]};
    p.dptr = (unsigned char*)depth->ptr;
    p.nptr = (unsigned char*)norm->ptr;
    p.iptr = (unsigned char*)img->ptr;
    p.dpitch = depth->pitch;
    p.npitch = norm->pitch;
    p.ipitch = img->pitch;
    p.w = (int)img->w; // the reference bounds the launch by img (cu_raycast.cu:39,110)
    p.h = (int)img->h;
    p.near = near;
    p.far = far;
    p.trunc = trunc_dist;
    p.subpix = subpix ? 1 : 0;
    p.nbx = (unsigned)geom.nbx;
    p.nby = (unsigned)geom.nby;
    p.cells = (const unsigned char*)cells;
    p.ccells = (const unsigned char*)color_cells;
    p.tab = brick_table_view(s + lay.tab, lay.t, n);
    p.ctab = brick_table_view(s + lay.ctab, lay.ct, n_color);
    if (p.w == 0 || p.h == 0) return 0;

    // raycast_launch's pixel tiling and its rule for small images (raycast.hip), under the same knobs
    static const int tile_env = env_int("KFX_RAYCAST_TILE", 5, 0, 6);
    static const int wg_env = env_int("KFX_RAYCAST_WG", 1, 0, 2);
    p.tile_log2w = tile_env;
    p.wg_log2x = wg_env;
    p.sparse_lanes = 0;
    dim3 grid(ceil_div(p.w, (1 << p.wg_log2x) << p.tile_log2w), ceil_div(p.h, (4 >> p.wg_log2x) * (64 >> p.tile_log2w)));
    static const int lanes_env = [] { const int v = env_int("KFX_RAYCAST_LANES", 0); return (v == 8 || v == 16 || v == 32) ? v : (v < 0 ? -1 : 0); }();
    const int lanes = lanes_env ? lanes_env : ((long long)p.w * p.h <= 160 * 120 ? 16 : 0);
    if (lanes && lanes_env >= 0) {
        p.sparse_lanes = lanes;
        grid = dim3(ceil_div(p.w, 2 * lanes), ceil_div(p.h, 2));
    }
    ColorGeom cv{};
    if (color) rb_frame_geometry(cv, frame);   // the colour frame: the SDF frame's dimensions and box
    const hipStream_t st = (hipStream_t)stream;
    if (color) hipLaunchKernelGGL((k_rb_raycast<RayF32, true>), grid, dim3(256), 0, st, p, cv);
    else if (cell == KFX_CELL_F32) hipLaunchKernelGGL((k_rb_raycast<RayF32, false>), grid, dim3(256), 0, st, p, cv);
    else hipLaunchKernelGGL((k_rb_raycast<RayF16, false>), grid, dim3(256), 0, st, p, cv);
    return check_launch(what);
}
