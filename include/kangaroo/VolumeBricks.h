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
#include <kfx_bricks.h>

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

}
