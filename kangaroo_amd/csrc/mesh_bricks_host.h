// mesh_bricks_host.h -- what mesh_bricks.hip (include/kfx_mesh_bricks.h) decides on the host before it launches anything: how the
// scratch is carved -- from the brick counts alone, never from the frame -- and the refusals of a scratch and of the outputs (the
// frame, the counts and the lists: bricks_host.h); and the same for the index scratch, the totals and the outputs of the indexed
// brick mesh (include/kfx_mesh_bricks_index.h).  No HIP in here: scripts/mesh_bricks_host_check.cpp and
// scripts/mesh_bricks_index_host_check.cpp drive it under the host sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/kfx_mesh_bricks.h"
#include "../../include/kfx_mesh_bricks_index.h"
#include "bricks_host.h"

namespace kfx {

constexpr int BRICK_NEIGHBOURS = 27;               // a brick and the 26 around it: slot (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
constexpr unsigned BRICK_MESH_BLOCK = 256;         // bricks per scan block

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

// the scratch (bricks_host.h's rule)
inline BrickRefusal brick_mesh_check_scratch(unsigned long long n, unsigned long long n_color, const void* scratch, size_t scratch_bytes)
{
    return brick_check_block(scratch, scratch_bytes, brick_mesh_scratch(n, n_color).bytes, "null scratch",
                             "scratch smaller than kfx_mesh_bricks_scratch_bytes()", "scratch not aligned to 256 bytes");
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

// ---- the indexed brick mesh (include/kfx_mesh_bricks_index.h) ----
constexpr unsigned BRICK_MESH_IDX_BLOCK = 256;                          // active cubes per scan block of an index plan
constexpr unsigned long long BRICK_MESH_MAX_TRIS = 4294967296ull / 3;   // 2^32 / 3: vertex offsets stay 32-bit

// The index scratch of an index plan and its emit (offsets in bytes from its start; include/kfx_mesh_bricks_index.h states the sum),
// for a list of n bricks and A = totals[0] active cubes:
//   hdr         256 bytes: words 0 .. 3 (8 bytes each) = vertices, triangles, and the active cubes and triangles it was planned for
//   cube_index  int64 per active cube: its dense index ci, in brick order
//   tri_offset  uint32 per active cube: its first triangle
//   info        uint32 per active cube: case flag | mask of the edges it owns << 8
//   vbase       uint32 per active cube: its first vertex id
//   first       uint32 per listed brick: the position of its first cube in cube_index (a brick without cubes: the next brick's)
//   part        2 uint32 per scan block of 256 cubes: its vertices, its triangles
//   base        2 uint64 per scan block: those before it
struct BrickMeshIndexScratch {
    size_t hdr, cube_index, tri_offset, info, vbase, first, part, base, bytes;
    unsigned long long nblk;
};
inline BrickMeshIndexScratch brick_mesh_index_scratch(unsigned long long n, unsigned long long n_active)
{
    BrickMeshIndexScratch s{};
    s.nblk = (n_active + BRICK_MESH_IDX_BLOCK - 1) / BRICK_MESH_IDX_BLOCK;
    s.hdr = 0;
    s.cube_index = 256;
    s.tri_offset = s.cube_index + brick_round256(8 * n_active);
    s.info = s.tri_offset + brick_round256(4 * n_active);
    s.vbase = s.info + brick_round256(4 * n_active);
    s.first = s.vbase + brick_round256(4 * n_active);
    s.part = s.first + brick_round256(4 * n);
    s.base = s.part + brick_round256(8 * s.nblk);
    s.bytes = s.base + brick_round256(16 * s.nblk);
    return s;
}

// totals a plan can have made, and a vertex count an index plan can have made of them
inline BrickRefusal brick_mesh_check_totals(const unsigned long long* totals, unsigned long long n_verts)
{
    if (!totals) return {KFX_E_NULL, "null totals"};
    if (totals[1] >= BRICK_MESH_MAX_TRIS || totals[0] > totals[1] || n_verts > 3 * totals[1]) return {KFX_E_RANGE, "totals out of range"};
    return {0, nullptr};
}
// the index scratch (bricks_host.h's rule); the totals are in range
inline BrickRefusal brick_mesh_index_check_scratch(unsigned long long n, const unsigned long long* totals, const void* index_scratch,
                                                   size_t index_scratch_bytes)
{
    return brick_check_block(index_scratch, index_scratch_bytes, brick_mesh_index_scratch(n, totals[0]).bytes, "null index scratch",
                             "index scratch smaller than kfx_mesh_bricks_index_scratch_bytes()", "index scratch not aligned to 256 bytes");
}
// the arrays of an indexed emit with cubes to write
inline BrickRefusal brick_mesh_check_indexed_outputs(const void* verts, const void* norms, const void* colors, const void* faces)
{
    if (!verts || !norms || !faces) return {KFX_E_NULL, "null output"};
    if (((uintptr_t)verts | (uintptr_t)norms | (uintptr_t)colors | (uintptr_t)faces) & 3) return {KFX_E_ALIGN, "output alignment"};
    return {0, nullptr};
}

} // namespace kfx
