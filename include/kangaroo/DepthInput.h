// DepthInput.h -- the start of the application's frame for C++ hosts (kfx_depth_input, include/kfx_sensor.h).  Addition beside
// the reference API: an upload ring that takes the sensor's raw image on the host and delivers the filtered depth image in
// metres, and BilateralFilterDepth, the stateless operator behind it.  Both carry the bits of
//   ElementwiseScaleBias<float, T, float>(metres, raw, s) followed by BilateralFilter<float, float>(filtered, metres, gs, gr, size, minval)
// (main.cpp:202-209).  Include it explicitly.
//
//   roo::DepthInput<unsigned short> input(w, h, 1.0f / 1000.0f);    // 2 slots: the copy of frame k + 1 runs beside frame k
//   roo::Image<unsigned short, roo::TargetHost, roo::DontManage> buf = input.Acquire();   // page-locked: the driver fills it
//   input.Submit();
//   input.Filter(dKinectFiltered, dKinectMeters, gs, gr, size, 0.2f);
#pragma once

#include <kangaroo/Image.h>
#include <kangaroo/platform.h>
#include <kangaroo/launch_utils.h>
#include <kfx_sensor.h>

namespace roo
{

namespace sensor_detail
{
template<typename T> struct Format;
template<> struct Format<unsigned short> { static const int value = KFX_DEPTH_U16; };
template<> struct Format<float> { static const int value = KFX_DEPTH_F32; };
}

// dFiltered = BilateralFilter(s * dRaw + offset), dMeters = s * dRaw + offset, one launch
template<typename T>
inline void BilateralFilterDepth(Image<float> dFiltered, Image<float> dMeters, const Image<T> dRaw, float s, float offset, float gs, float gr,
                                 uint size, float minval)
{
    GpuNoteStatus(kfx_bilateral_depth(dFiltered.abi(), dMeters.abi(), dRaw.abi(), sensor_detail::Format<T>::value, s, offset, gs, gr, size, minval, 0));
}
// ... without keeping the converted image
template<typename T>
inline void BilateralFilterDepth(Image<float> dFiltered, const Image<T> dRaw, float s, float offset, float gs, float gr, uint size, float minval)
{
    GpuNoteStatus(kfx_bilateral_depth(dFiltered.abi(), 0, dRaw.abi(), sensor_detail::Format<T>::value, s, offset, gs, gr, size, minval, 0));
}

template<typename T>
class DepthInput
{
public:
    DepthInput(size_t w, size_t h, float s, float offset = 0.f, int slots = 2) : handle_(0), w_(w), h_(h)
    {
        GpuCheckStatus(kfx_depth_input_create(&handle_, w, h, sensor_detail::Format<T>::value, s, offset, slots));
    }
    ~DepthInput() { if (handle_) kfx_depth_input_destroy(handle_); }
    DepthInput(const DepthInput&) = delete;
    DepthInput& operator=(const DepthInput&) = delete;

    // images submitted and not yet consumed by a Filter
    int Pending() const { return kfx_depth_input_pending(handle_); }
    // the next slot's host buffer (valid until Submit); a null image when the ring is full
    Image<T, TargetHost, DontManage> Acquire()
    {
        void* p = 0;
        size_t pitch = 0;
        if (kfx_depth_input_acquire(handle_, &p, &pitch) != 0) return Image<T, TargetHost, DontManage>();
        return Image<T, TargetHost, DontManage>((T*)p, w_, h_, pitch);
    }
    void Submit() { GpuCheckStatus(kfx_depth_input_submit(handle_)); }
    // the oldest pending image: dFiltered and (optionally) dMeters, on `stream`
    void Filter(Image<float> dFiltered, Image<float> dMeters, float gs, float gr, uint size, float minval, kfx_stream stream = 0)
    {
        GpuCheckStatus(kfx_depth_input_filter(handle_, dFiltered.abi(), dMeters.abi(), gs, gr, size, minval, stream));
    }
    void Filter(Image<float> dFiltered, float gs, float gr, uint size, float minval, kfx_stream stream = 0)
    {
        GpuCheckStatus(kfx_depth_input_filter(handle_, dFiltered.abi(), 0, gs, gr, size, minval, stream));
    }
    kfx_depth_input* get() const { return handle_; }

private:
    kfx_depth_input* handle_;
    size_t w_, h_;
};

}
