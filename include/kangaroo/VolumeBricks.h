// VolumeBricks.h -- sparse brick snapshots for C++ hosts (kfx_bricks_*, include/kfx_bricks.h).  Addition beside the reference API:
// the 8 x 8 x 8 bricks of a BoundedVolume -- or of any view of one -- that differ bitwise from the fill cell, packed on the device,
// and the way back.  Include it explicitly.
//
//   fill: for SDF_t / SDF_h what SdfReset(vol, fill) writes (the application: NaN), for a BoundedVolume<float> colour volume fill
//   itself (0.5).  Brick id = (bz * nby + by) * nbx + bx over the view's own grid of ceil(dim / 8) bricks per axis.
//
//   roo::Image<unsigned char, roo::TargetDevice, roo::Manage> scratch(roo::BrickScratchBytes(vol), 1);
//   const size_t n = roo::BrickPlan(vol, NAN, scratch.ptr, scratch.w);              // blocks until the count is on the host
//   roo::Image<unsigned, roo::TargetDevice, roo::Manage> ids(n ? n : 1, 1);
//   roo::Image<unsigned char, roo::TargetDevice, roo::Manage> cells((n ? n : 1) * roo::BrickBytes(vol), 1);
//   roo::BrickPack(vol, NAN, scratch.ptr, scratch.w, n, ids.ptr, cells.ptr);       // the volume unchanged since the plan
//   ...
//   roo::BrickUnpack(vol, ids.ptr, cells.ptr, n);                                  // those bricks' cells, and nothing else
//
// Errors: as SdfReset (launch_utils.h) -- a refused argument or a failed launch ends the process with the library's message.
#pragma once

#include <kangaroo/BoundedVolume.h>
#include <kangaroo/Sdf.h>
#include <kangaroo/VolumeShift.h>
#include <kangaroo/launch_utils.h>
#include <kangaroo/MarchingCubes.h>
#include <kangaroo/cu_raycast.h>
#include <kfx_bricks.h>
#include <kfx_mesh_bricks.h>
#include <kfx_mesh_bricks_index.h>
#include <kfx_raycast_bricks.h>
#include <kfx_brick_pool.h>

namespace roo
{

// bytes of one packed brick: 512 cells
template<typename T, typename M>
inline size_t BrickBytes(const BoundedVolume<T, TargetDevice, M>&) { return 512 * sizeof(T); }

template<typename T, typename M>
inline size_t BrickScratchBytes(const BoundedVolume<T, TargetDevice, M>& vol)
{
    return kfx_bricks_scratch_bytes(vol.abi(), shift_detail::Cell<T>::kind);
}

// the number of live bricks; the scratch then belongs to the BrickPack that follows
template<typename T, typename M>
inline size_t BrickPlan(const BoundedVolume<T, TargetDevice, M>& vol, float fill, void* scratch, size_t scratch_bytes)
{
    unsigned long long n = 0;
    GpuCheckStatus(kfx_bricks_plan(vol.abi(), shift_detail::Cell<T>::kind, fill, scratch, scratch_bytes, &n, 0));
    return (size_t)n;
}

template<typename T, typename M>
inline void BrickPack(const BoundedVolume<T, TargetDevice, M>& vol, float fill, const void* scratch, size_t scratch_bytes, size_t n_live, unsigned* ids,
                      void* cells)
{
    GpuCheckStatus(kfx_bricks_pack(vol.abi(), shift_detail::Cell<T>::kind, fill, scratch, scratch_bytes, n_live, ids, cells, 0));
}

template<typename T, typename M>
inline void BrickUnpack(BoundedVolume<T, TargetDevice, M>& vol, const unsigned* ids, const void* cells, size_t n)
{
    GpuCheckStatus(kfx_bricks_unpack(vol.abi(), shift_detail::Cell<T>::kind, ids, cells, n, 0));
}

// ---- the brick pool (kfx_brick_pool_*, include/kfx_brick_pool.h): device memory of the caller that keeps the live bricks a moving
// volume leaves behind under world brick keys, and gives them back; spill and restore are launches on the stream, nothing on the host.
// T is the cell type of the volumes the pool serves -- SDF_t, SDF_h or float -- deduced where a volume is an argument.  key0: the world
// key of the view's brick (0, 0, 0).
//
//   const size_t cap = 4096, bytes = roo::BrickPoolBytes<roo::SDF_t>(cap);
//   roo::Image<unsigned char, roo::TargetDevice, roo::Manage> pool(bytes, 1), scratch(roo::BrickPoolScratchBytes(vol, cap), 1);
//   roo::BrickPoolInit<roo::SDF_t>(pool.ptr, bytes, cap);
//   roo::BrickPoolSpill(pool.ptr, bytes, cap, vol.SubVolume(...), NAN, key0, scratch.ptr, scratch.w);      // before the shift
//   roo::BrickPoolRestore(pool.ptr, bytes, cap, vol.SubVolume(...), key1, scratch.ptr, scratch.w);         // after it
//   unsigned long long st[4]; roo::BrickPoolStats<roo::SDF_t>(pool.ptr, bytes, cap, st);                   // {occupied, spilled, restored, dropped}

template<typename T>
inline size_t BrickPoolBytes(size_t capacity) { return kfx_brick_pool_bytes(shift_detail::Cell<T>::kind, capacity); }

template<typename T, typename M>
inline size_t BrickPoolScratchBytes(const BoundedVolume<T, TargetDevice, M>& view, size_t capacity)
{
    return kfx_brick_pool_scratch_bytes(view.abi(), shift_detail::Cell<T>::kind, capacity);
}

template<typename T>
inline void BrickPoolInit(void* pool, size_t pool_bytes, size_t capacity)
{
    GpuCheckStatus(kfx_brick_pool_init(pool, pool_bytes, shift_detail::Cell<T>::kind, capacity, 0));
}

template<typename T, typename M>
inline void BrickPoolSpill(void* pool, size_t pool_bytes, size_t capacity, const BoundedVolume<T, TargetDevice, M>& view, float fill, const int key0[3],
                           void* scratch, size_t scratch_bytes)
{
    GpuCheckStatus(kfx_brick_pool_spill(pool, pool_bytes, shift_detail::Cell<T>::kind, capacity, view.abi(), fill, key0, scratch, scratch_bytes, 0));
}

template<typename T, typename M>
inline void BrickPoolRestore(void* pool, size_t pool_bytes, size_t capacity, const BoundedVolume<T, TargetDevice, M>& view, const int key0[3], void* scratch,
                             size_t scratch_bytes)
{
    GpuCheckStatus(kfx_brick_pool_restore(pool, pool_bytes, shift_detail::Cell<T>::kind, capacity, view.abi(), key0, scratch, scratch_bytes, 0));
}

// blocking: out = {occupied, spilled, restored, dropped}
template<typename T>
inline void BrickPoolStats(const void* pool, size_t pool_bytes, size_t capacity, unsigned long long out[4])
{
    GpuCheckStatus(kfx_brick_pool_stats(pool, pool_bytes, shift_detail::Cell<T>::kind, capacity, out, 0));
}

// cells_out[i] = the 512 cells of slot slots[i] (device lists)
template<typename T>
inline void BrickPoolGather(const void* pool, size_t pool_bytes, size_t capacity, const unsigned* slots, size_t n, void* cells_out)
{
    GpuCheckStatus(kfx_brick_pool_gather(pool, pool_bytes, shift_detail::Cell<T>::kind, capacity, slots, n, cells_out, 0));
}

// ---- the mesh of packed bricks (kfx_mesh_bricks_*, include/kfx_mesh_bricks.h): SaveMesh's mesh of the volume the bricks would unpack
// into -- NaN where no brick is listed, colour 0.5 -- without that volume.  The frame is the virtual volume's dimensions and box; `cell`
// is KFX_CELL_F32 or KFX_CELL_F16, the kind of the bricks in `cells`.
//
//   const kfx_volume frame = roo::BrickFrame(w, h, d, boxmin, boxmax);
//   roo::SaveMeshBricks("world", frame, KFX_CELL_F32, ids.ptr, cells.ptr, n);                         // -> world.ply
//   roo::SaveMeshBricks("world", frame, KFX_CELL_F32, ids.ptr, cells.ptr, n, cids.ptr, ccells.ptr, nc);   // with colours
//   roo::SaveMeshBricksIndexed("world", frame, KFX_CELL_F32, ids.ptr, cells.ptr, n);                  // one vertex per lattice edge, a face list

// a frame: only the dimensions and the box of the kfx_volume are read
inline kfx_volume BrickFrame(size_t w, size_t h, size_t d, float3 boxmin, float3 boxmax)
{
    kfx_volume f = {};
    f.w = w; f.h = h; f.d = d;
    f.boxmin[0] = boxmin.x; f.boxmin[1] = boxmin.y; f.boxmin[2] = boxmin.z;
    f.boxmax[0] = boxmax.x; f.boxmax[1] = boxmax.y; f.boxmax[2] = boxmax.z;
    return f;
}

inline size_t MeshBricksScratchBytes(size_t n, size_t n_color = 0) { return kfx_mesh_bricks_scratch_bytes(n, n_color); }

// totals[0] = active cubes, totals[1] = triangles; the scratch then belongs to the MeshBricksEmit that follows
inline void MeshBricksPlan(const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n, void* scratch, size_t scratch_bytes,
                           unsigned long long totals[2])
{
    GpuCheckStatus(kfx_mesh_bricks_plan(&frame, cell, ids, cells, n, scratch, scratch_bytes, totals, 0));
}

inline void MeshBricksEmit(const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n, const unsigned* color_ids,
                           const void* color_cells, size_t n_color, void* scratch, size_t scratch_bytes, const unsigned long long totals[2],
                           long long* cube_index, unsigned* tri_offset, float* verts, float* norms, float* colors)
{
    GpuCheckStatus(kfx_mesh_bricks_emit(&frame, cell, ids, cells, n, color_ids, color_cells, n_color, scratch, scratch_bytes, totals, cube_index,
                                        tri_offset, verts, norms, colors, 0));
}

// ---- the same mesh welded by lattice edge on the device (kfx_mesh_bricks_index_*, include/kfx_mesh_bricks_index.h): after MeshBricksPlan,
// with its scratch unchanged and its totals.
inline size_t MeshBricksIndexScratchBytes(size_t n, const unsigned long long totals[2]) { return kfx_mesh_bricks_index_scratch_bytes(n, totals); }

// the number of vertices V; the index scratch then belongs to the MeshBricksEmitIndexed that follows
inline size_t MeshBricksIndexPlan(const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n, const void* scratch,
                                  size_t scratch_bytes, const unsigned long long totals[2], void* index_scratch, size_t index_scratch_bytes)
{
    unsigned long long nvert = 0;
    GpuCheckStatus(kfx_mesh_bricks_index_plan(&frame, cell, ids, cells, n, scratch, scratch_bytes, totals, index_scratch, index_scratch_bytes, &nvert, 0));
    return (size_t)nvert;
}

// verts[V][3], norms[V][3], colors[V][4] or null, faces[T][3]
inline void MeshBricksEmitIndexed(const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n, const unsigned* color_ids,
                                  const void* color_cells, size_t n_color, void* scratch, size_t scratch_bytes, const void* index_scratch,
                                  size_t index_scratch_bytes, const unsigned long long totals[2], size_t n_verts, float* verts, float* norms,
                                  float* colors, unsigned* faces)
{
    GpuCheckStatus(kfx_mesh_bricks_emit_indexed(&frame, cell, ids, cells, n, color_ids, color_cells, n_color, scratch, scratch_bytes, index_scratch,
                                                index_scratch_bytes, totals, n_verts, verts, norms, colors, faces, 0));
}

namespace mesh_detail
{
// The brick mesh as host arrays (MarchingCubes.h's Extract over the brick lists): the soup, or with `indexed` its weld by lattice
// edge.  cube_index and tri_offset, if given, receive every active cube's dense index and first triangle in the list's order (soup).
inline HostMesh ExtractBricks(const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n, const unsigned* color_ids,
                              const void* color_cells, size_t n_color, bool color, bool indexed = false, std::vector<long long>* cube_index = nullptr,
                              std::vector<unsigned>* tri_offset = nullptr, const MeshKeep& keep = MeshKeep(), float simplify_cell = 0.0f,
                              int smooth_iterations = 0)
{
    const size_t nbytes = MeshBricksScratchBytes(n, color ? n_color : 0);
    DeviceBuffer scratch(nbytes), xscratch, active, offsets, faces;
    unsigned long long totals[2] = {0, 0};
    MeshBricksPlan(frame, cell, ids, cells, n, scratch.get(), nbytes, totals);
    HostMesh m;
    m.ntri = totals[1];
    m.nvert = 3 * m.ntri;
    m.color = color && frame.w >= 8 && frame.h >= 8 && frame.d >= 8;
    size_t xbytes = 0;
    if (indexed) {
        xbytes = MeshBricksIndexScratchBytes(n, totals);
        xscratch = DeviceBuffer(xbytes);
        m.nvert = MeshBricksIndexPlan(frame, cell, ids, cells, n, scratch.get(), nbytes, totals, xscratch.get(), xbytes);
        m.faces.resize(3 * m.ntri);
        faces = DeviceBuffer(m.faces.size() * 4);
    } else {
        active = DeviceBuffer(totals[0] * 8);
        offsets = DeviceBuffer(totals[0] * 4);
    }
    size_t nv = m.nvert;
    DeviceBuffer dv(nv * 12), dn(nv * 12), dc;
    if (m.color) dc = DeviceBuffer(nv * 16);
    const unsigned* const cids = m.color ? color_ids : nullptr;
    const void* const ccells = m.color ? color_cells : nullptr;
    const size_t nc = m.color ? n_color : 0;
    if (totals[0] && indexed)   // (the indexed emit reads the plan's scratch too: the bricks' neighbours)
        MeshBricksEmitIndexed(frame, cell, ids, cells, n, cids, ccells, nc, scratch.get(), nbytes, xscratch.get(), xbytes, totals, nv, dv.get<float>(),
                              dn.get<float>(), dc.get<float>(), faces.get<unsigned>());
    else if (totals[0])
        MeshBricksEmit(frame, cell, ids, cells, n, cids, ccells, nc, scratch.get(), nbytes, totals, active.get<long long>(), offsets.get<unsigned>(),
                       dv.get<float>(), dn.get<float>(), dc.get<float>());
    if (keep && indexed && m.ntri) {   // (MarchingCubes.h: the indexed mesh without its small components)
        FilterBuffers(dv, dn, dc, faces, nv, m.ntri, keep);
        m.nvert = nv;
        m.faces.resize(3 * m.ntri);
    }
    if (simplify_cell != 0.0f && indexed && m.ntri) {   // (... and then simplified on a grid of that cell, anchored at the world origin)
        SimplifyBuffers(dv, dn, dc, faces, nv, m.ntri, simplify_cell);
        m.nvert = nv;
        m.faces.resize(3 * m.ntri);
    }
    if (smooth_iterations != 0 && indexed && m.ntri) {   // (... and then smoothed, the normals recomputed from the faces)
        MeshSmoothing how;
        how.iterations = smooth_iterations;
        SmoothBuffers(dv, dn, faces, nv, m.ntri, how);
    }
    m.v.resize(nv * 3); m.n.resize(nv * 3); m.c.resize(m.color ? nv * 4 : 0);
    dv.CopyTo(m.v.data(), nv * 12);
    dn.CopyTo(m.n.data(), nv * 12);
    dc.CopyTo(m.c.data(), m.c.size() * 4);
    faces.CopyTo(m.faces.data(), m.faces.size() * 4);
    if (cube_index && !indexed) { cube_index->resize(totals[0]); active.CopyTo(cube_index->data(), totals[0] * 8); }
    if (tri_offset && !indexed) { tri_offset->resize(totals[0]); offsets.CopyTo(tri_offset->data(), totals[0] * 4); }
    return m;
}
}

// SaveMeshBricks(filename, frame, cell, ids, cells, n[, color_ids, color_cells, n_color]): <filename>.ply through SaveMesh's writer;
// returns the number of triangles written
inline size_t SaveMeshBricks(std::string filename, const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n)
{
    return mesh_detail::WritePly(filename + ".ply", mesh_detail::ExtractBricks(frame, cell, ids, cells, n, nullptr, nullptr, 0, false));
}

inline size_t SaveMeshBricks(std::string filename, const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n,
                             const unsigned* color_ids, const void* color_cells, size_t n_color)
{
    return mesh_detail::WritePly(filename + ".ply", mesh_detail::ExtractBricks(frame, cell, ids, cells, n, color_ids, color_cells, n_color, true));
}

// SaveMeshBricksIndexed(filename, frame, cell, ids, cells, n[, color_ids, color_cells, n_color]): SaveMeshBricks' mesh welded by lattice edge
// -- its first-occurrence vertices and a face list in its triangle order.  Returns the number of triangles written; nvert, if given,
// receives the number of vertices.
inline size_t SaveMeshBricksIndexed(std::string filename, const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n,
                                    size_t* nvert = nullptr)
{
    const mesh_detail::HostMesh m = mesh_detail::ExtractBricks(frame, cell, ids, cells, n, nullptr, nullptr, 0, false, true);
    if (nvert) *nvert = m.nvert;
    return mesh_detail::WritePly(filename + ".ply", m);
}

inline size_t SaveMeshBricksIndexed(std::string filename, const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n,
                                    const unsigned* color_ids, const void* color_cells, size_t n_color, size_t* nvert = nullptr)
{
    const mesh_detail::HostMesh m = mesh_detail::ExtractBricks(frame, cell, ids, cells, n, color_ids, color_cells, n_color, true, true);
    if (nvert) *nvert = m.nvert;
    return mesh_detail::WritePly(filename + ".ply", m);
}

// ... min_faces, largest: without its small components, filtered on the device (MarchingCubes.h: SaveMeshIndexed's); simplify_cell > 0:
// then simplified on a grid of that cell anchored at the world origin (include/kfx_mesh_simplify.h), 0: off; smooth_iterations > 0: then
// smoothed by that many Taubin iterations, the normals recomputed from the faces (include/kfx_mesh_smooth.h), 0: off
inline size_t SaveMeshBricksIndexed(std::string filename, const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n,
                                    size_t min_faces, bool largest, size_t* nvert = nullptr, float simplify_cell = 0.0f, int smooth_iterations = 0)
{
    const mesh_detail::HostMesh m = mesh_detail::ExtractBricks(frame, cell, ids, cells, n, nullptr, nullptr, 0, false, true, nullptr, nullptr,
                                                               mesh_detail::MeshKeep{min_faces, largest}, simplify_cell, smooth_iterations);
    if (nvert) *nvert = m.nvert;
    return mesh_detail::WritePly(filename + ".ply", m);
}

inline size_t SaveMeshBricksIndexed(std::string filename, const kfx_volume& frame, int cell, const unsigned* ids, const void* cells, size_t n,
                                    const unsigned* color_ids, const void* color_cells, size_t n_color, size_t min_faces, bool largest,
                                    size_t* nvert = nullptr, float simplify_cell = 0.0f, int smooth_iterations = 0)
{
    const mesh_detail::HostMesh m = mesh_detail::ExtractBricks(frame, cell, ids, cells, n, color_ids, color_cells, n_color, true, true, nullptr,
                                                               nullptr, mesh_detail::MeshKeep{min_faces, largest}, simplify_cell, smooth_iterations);
    if (nvert) *nvert = m.nvert;
    return mesh_detail::WritePly(filename + ".ply", m);
}

// ---- RaycastSdf of packed bricks (kfx_raycast_bricks_*, include/kfx_raycast_bricks.h): RaycastSdf's images of the volume the bricks
// would unpack into -- NaN where no brick is listed, colour 0.5 -- without that volume, bit for bit.  One plan serves any number of views.
//
//   roo::Image<unsigned char, roo::TargetDevice, roo::Manage> plan(roo::RaycastBricksScratchBytes(n), 1);
//   roo::RaycastBricksPlan(frame, ids.ptr, n, plan.ptr, plan.w);                                     // no read-back
//   roo::RaycastSdfBricks(depth, norm, img, frame, KFX_CELL_F32, ids.ptr, cells.ptr, n, plan.ptr, plan.w, T_wc, K, near, far, trunc, true);

inline size_t RaycastBricksScratchBytes(size_t n, size_t n_color = 0) { return kfx_raycast_bricks_scratch_bytes(n, n_color); }

inline void RaycastBricksPlan(const kfx_volume& frame, const unsigned* ids, size_t n, void* scratch, size_t scratch_bytes)
{
    GpuCheckStatus(kfx_raycast_bricks_plan(&frame, ids, n, nullptr, 0, scratch, scratch_bytes, 0));
}

inline void RaycastBricksPlan(const kfx_volume& frame, const unsigned* ids, size_t n, const unsigned* color_ids, size_t n_color, void* scratch,
                              size_t scratch_bytes)
{
    GpuCheckStatus(kfx_raycast_bricks_plan(&frame, ids, n, color_ids, n_color, scratch, scratch_bytes, 0));
}

inline void RaycastSdfBricks(Image<float> depth, Image<float4> norm, Image<float> img, const kfx_volume& frame, int cell, const unsigned* ids,
                             const void* cells, size_t n, const void* scratch, size_t scratch_bytes, const Mat<float, 3, 4> T_wc, ImageIntrinsics K,
                             float near, float far, float trunc_dist, bool subpix = true)
{
    GpuCheckStatus(kfx_raycast_bricks(depth.abi(), norm.abi(), img.abi(), &frame, cell, ids, cells, n, nullptr, nullptr, 0, 0, scratch, scratch_bytes,
                                      T_wc.m, &K.fu, near, far, trunc_dist, subpix ? 1 : 0, 0));
}

// the colour overload: img = the colour bricks' trilinear sample at the hit, 0.5 where no colour brick is listed (fp32 SDF cells)
inline void RaycastSdfBricks(Image<float> depth, Image<float4> norm, Image<float> img, const kfx_volume& frame, const unsigned* ids, const void* cells,
                             size_t n, const unsigned* color_ids, const void* color_cells, size_t n_color, const void* scratch, size_t scratch_bytes,
                             const Mat<float, 3, 4> T_wc, ImageIntrinsics K, float near, float far, float trunc_dist, bool subpix = true)
{
    GpuCheckStatus(kfx_raycast_bricks(depth.abi(), norm.abi(), img.abi(), &frame, KFX_CELL_F32, ids, cells, n, color_ids, color_cells, n_color, 1,
                                      scratch, scratch_bytes, T_wc.m, &K.fu, near, far, trunc_dist, subpix ? 1 : 0, 0));
}

}
