// VolumeShift.h -- moving volume for C++ hosts (kfx_volume_shift, include/kfx_shift.h).  Addition beside the reference API: shift
// the cells of a BoundedVolume -- or of any view of one -- by whole voxels, in place on the device, and move its box with them, so
// that the volume can follow the camera without a round trip through the host.  Include it explicitly.
//
//   new(x, y, z) = old(x + sx, y + sy, z + sz) where that cell lies inside the view, the fill elsewhere: for SDF_t / SDF_h what
//   SdfReset(vol, fill) writes (the application: NaN), for a BoundedVolume<float> colour volume fill itself (0.5).
//
//   const int3 s = make_int3(8, 0, -8);
//   roo::Image<unsigned char, roo::TargetDevice, roo::Manage> scratch(roo::VolumeShiftScratchBytes(vol, 8, 0, 0), 1);   // 16 planes
//   roo::VolumeShift(vol, 8, 0, 0, NAN, scratch.ptr, scratch.w);   // vol.bbox has moved by 8 voxels along x
//
// A caller that keeps an SdfSummary of the volume calls summary.Rebuild() afterwards: the summary is keyed by the storage.
// Errors: as SdfReset (launch_utils.h) -- a refused argument or a failed launch ends the process with the library's message.
#pragma once

#include <kangaroo/BoundedVolume.h>
#include <kangaroo/Sdf.h>
#include <kangaroo/launch_utils.h>
#include <kfx_shift.h>

namespace roo
{

namespace shift_detail
{
template<typename T> struct Cell;
template<> struct Cell<SDF_t> { static const int kind = KFX_CELL_F32; };
template<> struct Cell<SDF_h> { static const int kind = KFX_CELL_F16; };
template<> struct Cell<float> { static const int kind = KFX_CELL_COLOR; };
}

// bytes of scratch for this shift that hold `planes` packed z-planes (at least the library's minimum; 0: the shift needs none)
template<typename T, typename M>
inline size_t VolumeShiftScratchBytes(const BoundedVolume<T, TargetDevice, M>& vol, int sx, int sy, int sz, size_t planes = 16)
{
    const int shift[3] = {sx, sy, sz};
    const size_t least = kfx_volume_shift_scratch_bytes(vol.abi(), shift_detail::Cell<T>::kind, shift);
    const size_t want = (planes < vol.d ? planes : vol.d) * vol.w * vol.h * sizeof(T);
    return least == 0 ? 0 : (want > least ? want : least);
}

template<typename T, typename M>
inline void VolumeShift(BoundedVolume<T, TargetDevice, M>& vol, int sx, int sy, int sz, float fill, void* scratch, size_t scratch_bytes)
{
    const int shift[3] = {sx, sy, sz};
    if (sx == 0 && sy == 0 && sz == 0) return;
    float bmin[3], bmax[3];
    GpuCheckStatus(kfx_volume_shift_box(vol.abi(), shift, bmin, bmax));
    GpuCheckStatus(kfx_volume_shift(vol.abi(), shift_detail::Cell<T>::kind, shift, fill, scratch, scratch_bytes, 0));
    vol.bbox = BoundingBox(make_float3(bmin[0], bmin[1], bmin[2]), make_float3(bmax[0], bmax[1], bmax[2]));
}

}
