// sensor_host.h -- what preprocess.hip, sensor.hip and frame.hip share of the sensor input path (include/kfx_sensor.h).
#pragma once

#include "../../include/kfx_sensor.h"

namespace kfx {

// kfx_bilateral_depth; launch = false: its argument checks alone
int bilateral_depth(const kfx_image* filtered, const kfx_image* metres, const kfx_image* raw, int format, float s, float offset, float gs, float gr,
                    unsigned size, float minval, bool launch, kfx_stream stream);

// kfx_depth_input_filter in its two halves, for kfx_frame_step, which records its first timing event between them:
// `stream` waits for the oldest pending upload (nothing pending: KFX_E_RANGE) ...
int depth_input_wait(kfx_depth_input* in, kfx_stream stream);
// ... and the launch that consumes it (the wait enqueued before)
int depth_input_consume(kfx_depth_input* in, const kfx_image* filtered, const kfx_image* metres, float gs, float gr, unsigned size, float minval,
                        kfx_stream stream);
bool depth_input_matches(const kfx_depth_input* in, size_t w, size_t h);

} // namespace kfx
