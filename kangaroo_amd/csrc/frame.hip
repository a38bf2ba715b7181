// frame.hip -- kfx_frame (include/kfx.h): one frame of the reference application's loop
// (applications/kinectfusion/main.cpp:200-356, known poses) enqueued by ONE call.  Host code only: every launch goes through
// the library's own entry points (kfx_bilateral_f32, kfx_depth_to_vbo_normals_f32, kfx_sdf_fuse[_tracked],
// kfx_raycast_sdf[_tracked]), so a step writes exactly what the separate calls write; the point is the host side -- seven
// interpreter-level calls per 0.45 ms frame become one -- and device-event timing of the frame's parts that does not depend
// on the caller's runtime (torch's events see only torch's current stream).
#include <cmath>
#include <cstdlib>
#include <new>

#include "kfx_device.h"
#include "frame_host.h"
#include "sensor_host.h"
#include "shift_host.h"

struct kfx_frame {
    kfx_frame_config cfg;
    kfx_sdf_summary* summary;   // owned; created by the first set_track(1)
    int track;
    long long frames;           // steps so far
    kfx::EventRing ring;        // four events per frame: before preprocess, before SdfFuse, after SdfFuse, after RaycastSdf
    unsigned mask;              // which events the next steps record (kfx_frame_set_timing)
    kfx_image texels;           // (frame_host.h; a step that integrates without preprocessing lets kfx_sdf_fuse pack its own)
    kfx_depth_input* input;     // not owned (kfx_frame_set_input, include/kfx_sensor.h): where a step without `raw` takes its image from
};

using namespace kfx;

extern "C" int kfx_frame_create(kfx_frame** out, const kfx_frame_config* cfg)
{
    if (!out || !cfg) return set_error(KFX_E_NULL, "kfx_frame_create: null argument");
    *out = nullptr;
    if (!cfg->vol.ptr) return set_error(KFX_E_NULL, "kfx_frame_create: null volume");
    if (int e = check_frame_views(cfg->raw, cfg->filtered, cfg->vbo, cfg->normals, cfg->ray_depth, cfg->ray_norm, cfg->ray_img, "kfx_frame_create")) return e;
    if (cfg->timing_slots < 0 || cfg->timing_slots > (1 << 20)) return set_error(KFX_E_RANGE, "kfx_frame_create: timing_slots");
    kfx_frame* f = new (std::nothrow) kfx_frame;
    if (!f) return set_error(KFX_E_RANGE, "kfx_frame_create: out of memory");
    f->cfg = *cfg;
    f->summary = nullptr;
    f->track = 0;
    f->frames = 0;
    f->mask = KFX_FRAME_EVENTS_ALL;
    f->input = nullptr;
    f->texels = texel_image_alloc(cfg->filtered.w, cfg->filtered.h);
    if (int e = ring_create(f->ring, 4, cfg->timing_slots, -1, "kfx_frame_create")) {
        texel_image_free(f->texels);
        delete f;
        return e;
    }
    *out = f;
    return 0;
}

extern "C" int kfx_frame_destroy(kfx_frame* f)
{
    if (!f) return 0;
    if (f->summary) kfx_sdf_summary_destroy(f->summary);   // (synchronises the device)
    ring_destroy(f->ring);
    texel_image_free(f->texels);
    delete f;
    return 0;
}

// Which of a frame's four events the following steps record.  An event costs the stream a marker between two launches (four per
// frame: 2.7 % of a 0.42 ms frame, measured); a loop that only needs the SdfFuse window and the frame period records
// KFX_FRAME_EVENTS_FUSE.
extern "C" int kfx_frame_set_timing(kfx_frame* f, unsigned mask)
{
    if (!f) return set_error(KFX_E_NULL, "kfx_frame_set_timing: null frame");
    if (mask > KFX_FRAME_EVENTS_ALL) return set_error(KFX_E_RANGE, "kfx_frame_set_timing: mask");
    f->mask = mask;
    return 0;
}

extern "C" int kfx_frame_get_track(const kfx_frame* f) { return f ? f->track : set_error(KFX_E_NULL, "kfx_frame_get_track: null frame"); }
extern "C" kfx_sdf_summary* kfx_frame_summary(kfx_frame* f) { return f ? f->summary : nullptr; }
extern "C" long long kfx_frame_count(const kfx_frame* f) { return f ? f->frames : 0; }

// for kfx_frame_shift (shift.hip, shift_host.h)
kfx_volume* kfx::frame_volume(kfx_frame* f) { return &f->cfg.vol; }
kfx_sdf_summary* kfx::frame_tracked_summary(kfx_frame* f) { return f->track ? f->summary : nullptr; }

extern "C" int kfx_frame_set_track(kfx_frame* f, int on, kfx_stream stream)
{
    if (!f) return set_error(KFX_E_NULL, "kfx_frame_set_track: null frame");
    if (!on) {
        f->track = 0;   // the summary stays allocated and goes stale: the next set_track(1) rebuilds it
        return 0;
    }
    if (!f->summary)
        if (int e = kfx_sdf_summary_create(&f->summary, &f->cfg.vol)) return e;
    if (!f->track)
        if (int e = kfx_sdf_summary_rebuild(f->summary, stream)) return e;
    f->track = 1;
    return 0;
}

extern "C" int kfx_frame_set_input(kfx_frame* f, kfx_depth_input* in)
{
    if (!f) return set_error(KFX_E_NULL, "kfx_frame_set_input: null frame");
    if (in && !depth_input_matches(in, f->cfg.filtered.w, f->cfg.filtered.h)) return set_error(KFX_E_SHAPE, "kfx_frame_set_input: the ring's image size differs from the frame's");
    f->input = in;
    return 0;
}

// SdfReset(vol, NaN): "never observed" = (NaN, 0) (main.cpp:229); images pending in an attached upload ring stay pending
extern "C" int kfx_frame_reset(kfx_frame* f, kfx_stream stream)
{
    if (!f) return set_error(KFX_E_NULL, "kfx_frame_reset: null frame");
    const float nan = __builtin_nanf("");
    if (f->track) return kfx_sdf_reset_tracked(&f->cfg.vol, f->summary, nan, stream);
    return kfx_sdf_reset(&f->cfg.vol, nan, stream);
}

extern "C" int kfx_frame_step(kfx_frame* f, const kfx_image* raw, const float T_wc[12], const float* T_cw, unsigned parts, kfx_stream stream)
{
    if (!f || !T_wc) return set_error(KFX_E_NULL, "kfx_frame_step: null argument");
    if (parts == 0) parts = KFX_FRAME_PREPROCESS | KFX_FRAME_FUSE | KFX_FRAME_RAYCAST;
    const kfx_frame_config& c = f->cfg;
    const kfx_image* src = raw ? raw : &c.raw;
    float inv[12];
    if (!T_cw) {
        se3_inverse(T_wc, inv);
        T_cw = inv;
    }
    // the sensor image of this step: the oldest pending upload, which the stream waits for BEFORE the first timing event (the
    // preprocess span stays kernel time; a late upload lengthens the period)
    kfx_depth_input* const sensor = (!raw && (parts & KFX_FRAME_PREPROCESS)) ? f->input : nullptr;
    if (sensor)
        if (int e0 = depth_input_wait(sensor, stream)) return e0;
    ring_begin(f->ring, f->frames, f->mask);
    int e = 0;
    const auto record = [&](int k) {   // (a failed record is reported, the frame stops)
        const hipError_t he = ring_record(f->ring, f->frames, k, (hipStream_t)stream);
        if (he != hipSuccess && !e) e = set_error((int)he, "kfx_frame_step: hipEventRecord");
    };
    record(0);
    // the packed texels travel from this step's preprocess to this step's SdfFuse only (nobody else can have touched the maps in between)
    const kfx_image* tex = ((parts & KFX_FRAME_PREPROCESS) && (parts & KFX_FRAME_FUSE) && f->texels.ptr) ? &f->texels : nullptr;
    if (!e && (parts & KFX_FRAME_PREPROCESS)) {
        if (sensor) e = depth_input_consume(sensor, &c.filtered, &c.raw, c.bilateral_gs, c.bilateral_gr, c.bilateral_size, c.bilateral_minval, stream);
        else e = kfx_bilateral_f32(&c.filtered, src, c.bilateral_gs, c.bilateral_gr, c.bilateral_size, c.bilateral_minval, 1, stream);
        if (!e) e = depth_to_vbo_normals_texels(&c.vbo, &c.normals, &c.filtered, c.K, 1.0f, tex, stream);
    }
    record(1);
    if (!e && (parts & KFX_FRAME_FUSE))
        e = sdf_fuse_texels(&c.vol, f->track ? f->summary : nullptr, &c.filtered, &c.normals, tex, T_cw, c.K, c.trunc_dist, c.max_w, c.mincostheta, c.fuse_flags, stream);
    record(2);
    if (!e && (parts & KFX_FRAME_RAYCAST)) {
        if (f->track) e = kfx_raycast_sdf_tracked(&c.ray_depth, &c.ray_norm, &c.ray_img, &c.vol, f->summary, T_wc, c.K, c.near, c.far, c.trunc_dist, 1, stream);
        else e = kfx_raycast_sdf(&c.ray_depth, &c.ray_norm, &c.ray_img, &c.vol, T_wc, c.K, c.near, c.far, c.trunc_dist, 1, stream);
    }
    record(3);
    f->frames += 1;
    return e;
}

// preprocess, SdfFuse, RaycastSdf, the three together, the period to the next frame
static void frame_spans(const EventRing& r, long long fr, float* o, hipError_t& he)
{
    o[0] = ring_span(r, fr, 0, 1, he);
    o[1] = ring_span(r, fr, 1, 2, he);
    o[2] = ring_span(r, fr, 2, 3, he);
    o[3] = ring_span(r, fr, 0, 3, he);
    o[4] = ring_period(r, fr, he);
}

extern "C" int kfx_frame_timings(kfx_frame* f, long long first_frame, int n_frames, float* ms)
{
    if (!f || !ms) return set_error(KFX_E_NULL, "kfx_frame_timings: null argument");
    return ring_timings(f->ring, f->frames, first_frame, n_frames, KFX_FRAME_TIMING_FIELDS, ms, frame_spans, "kfx_frame_timings");
}
