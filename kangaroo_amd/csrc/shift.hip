// shift.hip -- kfx_volume_shift (include/kfx_shift.h): move the cells of a volume by whole voxels, in place.  The plan -- which
// launches, in which order, and why none of them reads what it writes -- is shift_host.h's; this file holds the one row-copy kernel
// all four kinds of step run and the entry points.
//
// A pure streaming job: every cell is read once and written once (twice where a chunk is staged through the scratch).  A lane owns
// 16 bytes of a DESTINATION row, on a 16-byte boundary of the address space, and writes them with one nontemporal 16-byte store; the
// head and tail of a row that does not start or end on such a boundary (a sub-view) are written cell by cell, never beyond the
// view.  The source is read with one 16-byte load where the lane's cells all have a source and that source happens to lie on a
// 16-byte boundary too (always, when sx and the view's start keep the two rows mutually aligned), cell by cell otherwise.  No LDS,
// no atomics, nothing between workgroups: ordering comes from the stream.
#include <cstring>

#include <hip/hip_fp16.h>

#include "kfx_device.h"
#include "host_args.h"
#include "shift_host.h"

using namespace kfx;

typedef unsigned v4u __attribute__((ext_vector_type(4)));

template <int CELL> struct ShiftCell;
template <> struct ShiftCell<4> { typedef unsigned T; };
template <> struct ShiftCell<8> { typedef unsigned long long T; };

struct ShiftArgs {
    unsigned char* dst;         // plane 0, row 0, cell 0 of the planes written
    const unsigned char* src;   // plane 0, row 0, cell 0 of the planes read (null: fill only)
    size_t dpitch, dimg, spitch, simg;
    int w, h;                   // cells per row, rows per plane (both buffers)
    int sx, sy;                 // dst(x, y) = src(x + sx, y + sy)
    unsigned nrows;             // planes * h
    unsigned long long fill;    // the cell's fill bytes (CELL 4: the low word)
};

// One wave per 1 KiB of a destination row and round: blockIdx.x picks the 1 KiB, the rows are a grid-stride loop.
template <int CELL>
__global__ __launch_bounds__(256) void k_shift_rows(const ShiftArgs a)
{
    typedef typename ShiftCell<CELL>::T cell_t;
    constexpr int CPS = 16 / CELL;   // cells per 16-byte segment
    const int lane = threadIdx.x & 63;
    const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const cell_t fill = (cell_t)a.fill;
    v4u fill4;
    if constexpr (CELL == 4) { fill4.x = fill4.y = fill4.z = fill4.w = (unsigned)a.fill; }
    else { fill4.x = fill4.z = (unsigned)a.fill; fill4.y = fill4.w = (unsigned)(a.fill >> 32); }
    const int seg = (int)blockIdx.x * 64 + lane;
    for (unsigned row = blockIdx.y * 4u + wave; row < a.nrows; row += gridDim.y * 4u) {
        const unsigned p = row / (unsigned)a.h;
        const int y = (int)(row - p * (unsigned)a.h);
        unsigned char* const drow = a.dst + (size_t)p * a.dimg + (size_t)y * a.dpitch;
        const int mis = (int)(((uintptr_t)drow & 15) / CELL);   // cells between the 16-byte boundary below the row and its first cell
        const int x0 = seg * CPS - mis;                          // the lane's first cell (may be -mis .. -1 in the row's head)
        if (x0 >= a.w) continue;
        const int ys = y + a.sy;
        const bool has_row = a.src != nullptr && (unsigned)ys < (unsigned)a.h;
        const unsigned char* const srow = a.src + (size_t)p * a.simg + (size_t)(has_row ? ys : 0) * a.spitch;
        const int xs0 = x0 + a.sx;
        if (x0 >= 0 && x0 + CPS <= a.w) {
            v4u v = fill4;
            if (has_row && xs0 + CPS > 0 && xs0 < a.w) {
                const unsigned char* const s = srow + (ptrdiff_t)xs0 * CELL;
                if (xs0 >= 0 && xs0 + CPS <= a.w && ((uintptr_t)s & 15) == 0) {
                    v = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(s));
                } else {
                    cell_t c[CPS];
#pragma unroll
                    for (int k = 0; k < CPS; ++k)
                        c[k] = (unsigned)(xs0 + k) < (unsigned)a.w ? __builtin_nontemporal_load(reinterpret_cast<const cell_t*>(s) + k) : fill;
                    if constexpr (CELL == 4) { v.x = c[0]; v.y = c[1]; v.z = c[2]; v.w = c[3]; }
                    else { v.x = (unsigned)c[0]; v.y = (unsigned)(c[0] >> 32); v.z = (unsigned)c[1]; v.w = (unsigned)(c[1] >> 32); }
                }
            }
            __builtin_nontemporal_store(v, reinterpret_cast<v4u*>(drow + (ptrdiff_t)x0 * CELL));
        } else {
            // the row's head or tail: only the cells inside the view
#pragma unroll
            for (int k = 0; k < CPS; ++k) {
                const int x = x0 + k, xs = xs0 + k;
                if ((unsigned)x >= (unsigned)a.w) continue;
                cell_t c = fill;
                if (has_row && (unsigned)xs < (unsigned)a.w) c = __builtin_nontemporal_load(reinterpret_cast<const cell_t*>(srow) + xs);
                reinterpret_cast<cell_t*>(drow)[x] = c;
            }
        }
    }
}

// the geometry both host entry points derive from their arguments, after the checks; 0 or the refusal
struct ShiftSetup {
    ShiftGeom g;
    size_t cb;
};
static int shift_setup(ShiftSetup& s, const kfx_volume* vol, int cell, const int shift[3], const char* what)
{
    if (!vol || !vol->ptr) return fail_rule(what, KFX_E_NULL, "null volume");
    if (!shift) return fail_rule(what, KFX_E_NULL, "null shift");
    s.cb = shift_cell_bytes(cell);
    if (!s.cb) return fail_rule(what, KFX_E_RANGE, "unknown cell kind");
    if (int e = check_volume(vol, s.cb, 1, VOLUME_MAX_DIM, what)) return e;
    s.g = ShiftGeom{(int)vol->w, (int)vol->h, (int)vol->d, shift[0], shift[1], shift[2], vol->w * vol->h * s.cb};
    return 0;
}
// the scratch of a plan that stages: present, aligned, at least one plane
static int shift_check_scratch(const ShiftGeom& g, const void* scratch, size_t scratch_bytes, bool need_ptr, const char* what)
{
    const size_t need = shift_min_scratch(g);
    if (!need) return 0;
    if (need_ptr && !scratch) return fail_rule(what, KFX_E_NULL, "null scratch");
    if (scratch_bytes < need) return fail_rule(what, KFX_E_SHAPE, "scratch smaller than one packed plane");
    if ((uintptr_t)scratch & 255) return fail_rule(what, KFX_E_ALIGN, "scratch not aligned to 256 bytes");
    return 0;
}

unsigned long long kfx::shift_fill_bytes(int cell, float fill)
{
    unsigned u;
    memcpy(&u, &fill, 4);
    if (cell == KFX_CELL_F16) return (unsigned long long)__half_as_ushort(__float2half_rn(fill));   // {val = fill, w = 0}: kfx_sdf_reset_h's pattern
    return (unsigned long long)u;                                                                    // F32: {fill, 0.0f}; colour: fill
}

static void shift_launch(const kfx_volume* vol, const ShiftSetup& s, const kfx_shift_step& st, unsigned long long fill, unsigned char* scratch, hipStream_t stream)
{
    const ShiftGeom& g = s.g;
    const size_t cb = s.cb, prow = (size_t)g.w * cb, pimg = prow * g.h;   // the packed layout of the scratch
    unsigned char* const base = (unsigned char*)vol->ptr;
    ShiftArgs a{};
    a.w = g.w; a.h = g.h;
    a.fill = fill;
    a.nrows = (unsigned)(st.dst_z1 - st.dst_z0) * (unsigned)g.h;
    if (st.kind == KFX_SHIFT_STAGE) {
        a.dst = scratch + (size_t)st.dst_z0 * pimg; a.dpitch = prow; a.dimg = pimg;
        a.src = base + (size_t)st.src_z0 * vol->img_pitch; a.spitch = vol->pitch; a.simg = vol->img_pitch;
    } else {
        a.dst = base + (size_t)st.dst_z0 * vol->img_pitch; a.dpitch = vol->pitch; a.dimg = vol->img_pitch;
        a.sx = g.sx; a.sy = g.sy;
        if (st.kind == KFX_SHIFT_DIRECT) { a.src = base + (size_t)st.src_z0 * vol->img_pitch; a.spitch = vol->pitch; a.simg = vol->img_pitch; }
        else if (st.kind == KFX_SHIFT_PLACE) { a.src = scratch + (size_t)st.src_z0 * pimg; a.spitch = prow; a.simg = pimg; }
    }
    if (!a.nrows) return;
    // 16-byte segments a row can touch: its bytes, plus the cells a row may start beyond a boundary where rows are not all aligned
    const bool aligned = (((uintptr_t)a.dst | a.dpitch | a.dimg) & 15) == 0;
    const size_t segs = (prow + (aligned ? 0 : 16 - cb) + 15) / 16;
    const unsigned gx = (unsigned)((segs + 63) / 64);
    const unsigned want = (a.nrows + 3) / 4, cap = gx >= 2048 ? 1u : 2048u / gx;   // ~2048 workgroups: 8 per CU
    const dim3 grid(gx, want < cap ? want : cap);
    if (cb == 8) hipLaunchKernelGGL(k_shift_rows<8>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_shift_rows<4>, grid, dim3(256), 0, stream, a);
}

extern "C" size_t kfx_volume_shift_scratch_bytes(const kfx_volume* vol, int cell, const int shift[3])
{
    ShiftSetup s;
    if (shift_setup(s, vol, cell, shift, "kfx_volume_shift_scratch_bytes")) return 0;
    return shift_min_scratch(s.g);
}

extern "C" int kfx_volume_shift_box(const kfx_volume* vol, const int shift[3], float boxmin_out[3], float boxmax_out[3])
{
    if (!vol || !shift || !boxmin_out || !boxmax_out) return set_error(KFX_E_NULL, "kfx_volume_shift_box: null argument");
    if (vol->w < 1 || vol->h < 1 || vol->d < 1) return set_error(KFX_E_SHAPE, "kfx_volume_shift_box: volume dimensions");
    shift_box(*vol, shift, boxmin_out, boxmax_out);
    return 0;
}

extern "C" int kfx_volume_shift_plan(const kfx_volume* vol, int cell, const int shift[3], size_t scratch_bytes, kfx_shift_step* steps_out, int max_steps,
                                     int* n_steps_out)
{
    ShiftSetup s;
    if (int e = shift_setup(s, vol, cell, shift, "kfx_volume_shift_plan")) return e;
    if (!n_steps_out || (max_steps > 0 && !steps_out)) return set_error(KFX_E_NULL, "kfx_volume_shift_plan: null argument");
    if (int e = shift_check_scratch(s.g, nullptr, scratch_bytes, false, "kfx_volume_shift_plan")) return e;
    *n_steps_out = shift_plan(s.g, s.g.plane_bytes ? scratch_bytes / s.g.plane_bytes : 0, [&](const kfx_shift_step& st) {
        if (max_steps > 0) { *steps_out++ = st; --max_steps; }
    });
    return 0;
}

extern "C" int kfx_volume_shift(const kfx_volume* vol, int cell, const int shift[3], float fill, void* scratch, size_t scratch_bytes, kfx_stream stream)
{
    ShiftSetup s;
    if (int e = shift_setup(s, vol, cell, shift, "kfx_volume_shift")) return e;
    if (int e = shift_check_scratch(s.g, scratch, scratch_bytes, true, "kfx_volume_shift")) return e;
    if (shift_is_zero(s.g)) return 0;
    const unsigned long long fb = shift_fill_bytes(cell, fill);
    const size_t planes = shift_is_staged(s.g) ? scratch_bytes / s.g.plane_bytes : 0;
    shift_plan(s.g, planes, [&](const kfx_shift_step& st) { shift_launch(vol, s, st, fb, (unsigned char*)scratch, (hipStream_t)stream); });
    return check_launch("kfx_volume_shift");
}

extern "C" int kfx_frame_shift(kfx_frame* frame, const int shift[3], void* scratch, size_t scratch_bytes, kfx_stream stream)
{
    if (!frame) return set_error(KFX_E_NULL, "kfx_frame_shift: null frame");
    kfx_volume* const vol = frame_volume(frame);
    float bmin[3], bmax[3];
    if (int e = kfx_volume_shift(vol, KFX_CELL_F32, shift, __builtin_nanf(""), scratch, scratch_bytes, stream)) return e;
    if (shift[0] == 0 && shift[1] == 0 && shift[2] == 0) return 0;   // nothing moved: the box stays what it is, bit for bit
    if (int e = kfx_volume_shift_box(vol, shift, bmin, bmax)) return e;
    memcpy(vol->boxmin, bmin, sizeof(bmin));
    memcpy(vol->boxmax, bmax, sizeof(bmax));
    // the summary is keyed by the storage and holds no box: what it says about the bricks is rebuilt from the moved cells
    if (kfx_sdf_summary* sum = frame_tracked_summary(frame)) return kfx_sdf_summary_rebuild(sum, stream);
    return 0;
}
