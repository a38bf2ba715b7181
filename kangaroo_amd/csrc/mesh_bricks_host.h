// mesh_bricks_host.h -- what mesh_bricks.hip (include/kfx_mesh_bricks.h) decides on the host before it launches anything: which frames
// it accepts and their brick grid, how the scratch is carved -- from the brick counts alone, never from the frame -- and the refusals of
// a scratch, of the brick lists and of the outputs.  No HIP in here: scripts/mesh_bricks_host_check.cpp drives it under the host
// sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kfx_mesh_bricks.h"
#include "bricks_host.h"

namespace kfx {

constexpr int BRICK_NEIGHBOURS = 27;               // a brick and the 26 around it: slot (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
constexpr unsigned BRICK_MESH_BLOCK = 256;         // bricks per scan block
constexpr size_t FRAME_MIN_DIM = 3, FRAME_MAX_DIM = 65535;   // the dimensions kfx_mesh_plan accepts of a dense volume

// The frame: a virtual dense volume, of which only the dimensions and the box are read.  Its brick grid in g.
inline BrickRefusal brick_mesh_check_frame(const kfx_volume* frame, int cell, BrickGeom& g)
{
    if (!frame) return {KFX_E_NULL, "null frame"};
    if (cell != KFX_CELL_F32 && cell != KFX_CELL_F16) return {KFX_E_RANGE, "unknown cell kind"};
    if (frame->w < FRAME_MIN_DIM || frame->h < FRAME_MIN_DIM || frame->d < FRAME_MIN_DIM || frame->w > FRAME_MAX_DIM ||
        frame->h > FRAME_MAX_DIM || frame->d > FRAME_MAX_DIM)
        return {KFX_E_SHAPE, "frame dimensions"};
    g = brick_geom(frame->w, frame->h, frame->d);
    return brick_check_grid(g);
}

// The scratch of a plan and its emit (offsets in bytes from its start; include/kfx_mesh_bricks.h states the sum):
//   hdr    256 bytes: words 0, 1 (8 bytes each) = active cubes, triangles
//   nbr    int32 per listed brick and neighbour: the neighbour's position in the list, -1 if it is not listed
//   cnt    uint32 per listed brick: active cubes << 16 | triangles (at most 512 and 2560)
//   part   2 uint32 per scan block: its active cubes, its triangles
//   base   2 uint64 per scan block: those before it
//   cnbr   with a colour list: int32 per listed brick and neighbour, the neighbour's position in the colour list or -1
// A plan carves with n_color = 0: its layout is the front of every emit's.
struct BrickMeshScratch {
    size_t hdr, nbr, cnt, part, base, cnbr, bytes;
    unsigned long long nblk;
};
inline BrickMeshScratch brick_mesh_scratch(unsigned long long n, unsigned long long n_color)
{
    BrickMeshScratch s{};
    s.nblk = (n + BRICK_MESH_BLOCK - 1) / BRICK_MESH_BLOCK;
    s.hdr = 0;
    s.nbr = 256;
    s.cnt = s.nbr + brick_round256(4ull * BRICK_NEIGHBOURS * n);
    s.part = s.cnt + brick_round256(4 * n);
    s.base = s.part + brick_round256(8 * s.nblk);
    s.cnbr = s.base + brick_round256(16 * s.nblk);
    s.bytes = s.cnbr + (n_color ? brick_round256(4ull * BRICK_NEIGHBOURS * n) : 0);
    return s;
}

inline BrickRefusal brick_mesh_check_counts(unsigned long long n, unsigned long long n_color)
{
    if (n > BRICK_MAX || n_color > BRICK_MAX) return {KFX_E_RANGE, "more than 2^31 - 1 entries"};
    return {0, nullptr};
}
// the scratch: present, large enough, aligned -- in that order (as bricks_host.h)
inline BrickRefusal brick_mesh_check_scratch(unsigned long long n, unsigned long long n_color, const void* scratch, size_t scratch_bytes)
{
    if (!scratch) return {KFX_E_NULL, "null scratch"};
    if (scratch_bytes < brick_mesh_scratch(n, n_color).bytes) return {KFX_E_SHAPE, "scratch smaller than kfx_mesh_bricks_scratch_bytes()"};
    if ((uintptr_t)scratch & 255) return {KFX_E_ALIGN, "scratch not aligned to 256 bytes"};
    return {0, nullptr};
}
// the arrays of an emit with cubes to write
inline BrickRefusal brick_mesh_check_outputs(const void* cube_index, const void* tri_offset, const void* verts, const void* norms, const void* colors)
{
    if (!cube_index || !tri_offset || !verts || !norms) return {KFX_E_NULL, "null output"};
    if (((uintptr_t)cube_index & 7) || (((uintptr_t)tri_offset | (uintptr_t)verts | (uintptr_t)norms | (uintptr_t)colors) & 3))
        return {KFX_E_ALIGN, "output alignment"};
    return {0, nullptr};
}

// colours are written when the caller asks for them and the frame IsValid(): every dimension >= 8 (BoundedVolume.h:84-87)
inline bool brick_mesh_has_color(const BrickGeom& g, const void* colors) { return colors && g.w >= 8 && g.h >= 8 && g.d >= 8; }

} // namespace kfx
