/* kfx_sensor.h -- the start of the application's frame (applications/kinectfusion/main.cpp:202-209): a raw sensor image on the
 * host becomes the filtered depth image in metres.  Same library (libkfx.so); kept out of kfx.h.
 *
 * Stateless operators
 *   kfx_elementwise_scale_bias_u16  roo::ElementwiseScaleBias<float, unsigned short, float>: out = s * in + offset.
 *   kfx_bilateral_depth             BilateralFilter(filtered, s * raw + offset, gs, gr, size, minval) in ONE launch: `raw` holds
 *                                   `format` pixels in sensor units, the window is filtered in metres (minval is compared in
 *                                   metres), and `metres` (may be NULL) receives s * raw + offset for the pixels of `filtered`.
 *                                   Both images carry the bits of ElementwiseScaleBias followed by kfx_bilateral_f32(..., minval,
 *                                   1, ...), in both numerics modes.  metres and raw cover filtered; raw may be larger (its own
 *                                   extent clamps the window, as in kfx_bilateral_f32).
 *
 * kfx_depth_input: an upload ring of 2..8 slots.  A slot is one page-locked host buffer (rows of w pixels, no padding), one pitched
 * staging image in device memory and two events, `uploaded` and `consumed`; the ring owns one non-blocking copy stream.
 *   acquire  the host buffer of the next slot, for the sensor driver to fill.  Every slot holding an image that no filter has
 *            consumed: KFX_E_RANGE ("ring full"), nothing changes -- decided from host counters.  A slot used before: the call
 *            first waits on the host for the slot's last `uploaded` event (that copy has left the buffer).  Acquiring twice without
 *            a submit hands out the same buffer.
 *   submit   on the copy stream: wait for the slot's `consumed` event of its previous use, copy host -> staging, record `uploaded`.
 *            Without an acquired buffer: KFX_E_RANGE.
 *   pending  images submitted and not yet consumed.
 *   filter   consumes the OLDEST pending image: `stream` waits for its `uploaded` event, kfx_bilateral_depth reads the staging
 *            image, `consumed` is recorded on `stream`.  Nothing pending: KFX_E_RANGE.  Refused image arguments leave the image
 *            pending.
 *   destroy  synchronises the copy stream, then frees.  The caller has synchronised the streams it gave to filter, and has
 *            detached the ring from any frame.  A null ring: KFX_E_NULL.
 * Every stream wait is on an event whose record was enqueued before; the only host wait is on `uploaded` events of submitted
 * copies.  One thread at a time per ring.
 *
 * kfx_frame_set_input(frame, in): a kfx_frame_step with raw == NULL and KFX_FRAME_PREPROCESS then runs filter into cfg.filtered
 * and cfg.raw (so cfg.raw holds the frame's depth in metres, as dKinectMeters does) instead of kfx_bilateral_f32(cfg.raw); the wait
 * for the upload is enqueued before the step's first timing event, so `preprocess` stays kernel time and a late upload shows in
 * `period`.  The ring's w x h must be the frame's.  A step with an explicit raw, or without KFX_FRAME_PREPROCESS, leaves the ring
 * alone, and so does kfx_frame_reset.  in == NULL detaches.
 *
 * Returns 0, KFX_E_*, or a hipError_t (> 0). */
#ifndef KFX_SENSOR_H
#define KFX_SENSOR_H

#include "kfx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KFX_DEPTH_U16 0   /* unsigned short, e.g. millimetres */
#define KFX_DEPTH_F32 1   /* float in sensor units */

int kfx_elementwise_scale_bias_u16(const kfx_image* out, const kfx_image* in, float s, float offset, kfx_stream stream);
int kfx_bilateral_depth(const kfx_image* filtered, const kfx_image* metres, const kfx_image* raw, int format, float s, float offset,
                        float gs, float gr, unsigned size, float minval, kfx_stream stream);

typedef struct kfx_depth_input kfx_depth_input;
int kfx_depth_input_create(kfx_depth_input** out, size_t w, size_t h, int format, float s, float offset, int slots);
int kfx_depth_input_destroy(kfx_depth_input* in);
int kfx_depth_input_acquire(kfx_depth_input* in, void** host_ptr, size_t* pitch);
int kfx_depth_input_submit(kfx_depth_input* in);
int kfx_depth_input_pending(const kfx_depth_input* in);
int kfx_depth_input_filter(kfx_depth_input* in, const kfx_image* filtered, const kfx_image* metres, float gs, float gr, unsigned size,
                           float minval, kfx_stream stream);

int kfx_frame_set_input(kfx_frame* frame, kfx_depth_input* in);

#ifdef __cplusplus
}
#endif
#endif /* KFX_SENSOR_H */
