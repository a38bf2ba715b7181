// frame_host.h -- what the two frame objects, kfx_frame (frame.hip) and kfx_slab_frame (slab_frame.hip), do alike on the host: the
// check of a configuration's image views, SE3inv of the camera pose, the owned packed-texel image, and the ring of timing events.
#pragma once

#include <new>

#include "kfx_device.h"
#include "host_args.h"

namespace kfx {

// The seven views of a frame configuration: each a usable, non-empty image (check_image), the preprocess images of one size.  A view
// without a pointer is a malformed configuration (KFX_E_SHAPE), not a null argument.
inline int check_frame_views(const kfx_image& raw, const kfx_image& filtered, const kfx_image& vbo, const kfx_image& normals, const kfx_image& ray_depth,
                             const kfx_image& ray_norm, const kfx_image& ray_img, const char* what)
{
    const struct { const kfx_image* im; size_t elem; } views[7] = {{&raw, 4}, {&filtered, 4}, {&vbo, 16}, {&normals, 16}, {&ray_depth, 4}, {&ray_norm, 16}, {&ray_img, 4}};
    for (const auto& v : views) {
        if (!v.im->ptr) return fail_rule(what, KFX_E_SHAPE, "image views");
        if (int e = check_image(v.im, v.elem, 1, 1, what)) return e;
    }
    if (filtered.w != raw.w || filtered.h != raw.h || vbo.w != raw.w || vbo.h != raw.h || normals.w != raw.w || normals.h != raw.h)
        return fail_rule(what, KFX_E_SHAPE, "the preprocess images differ in size");
    return 0;
}

// SE3inv: [R^T | -R^T t], evaluated in double and rounded once
inline void se3_inverse(const float T_wc[12], float out[12])
{
    for (int i = 0; i < 3; ++i) {
        double t = 0.0;
        for (int j = 0; j < 3; ++j) {
            out[i * 4 + j] = T_wc[j * 4 + i];
            t += (double)T_wc[j * 4 + i] * (double)T_wc[j * 4 + 3];
        }
        out[i * 4 + 3] = (float)-t;
    }
}

// The packed texel image {nx, ny, nz, depth} of a frame (host_args.h: tex_layout), owned by the frame object: written by the fused vbo /
// normals launch of a step, staged by LDS-DMA in the SdfFuse of the SAME step.  No device (the argument checks of tests/test_abi_cpu.py
// run without one) or no memory: a null image, and the SdfFuse packs per call instead.
inline kfx_image texel_image_alloc(size_t w, size_t h)
{
    const TexLayout tl = tex_layout(w, h);
    void* buf = nullptr;
    if (tl.tpitch < (1u << 24) && hipMalloc(&buf, tl.bytes) == hipSuccess) return kfx_image{tl.tpitch, buf, w, h};
    (void)hipGetLastError();
    return kfx_image{0, nullptr, 0, 0};
}
inline void texel_image_free(kfx_image& t)
{
    if (t.ptr) { (void)hipFree(t.ptr); (void)hipGetLastError(); }
    t = kfx_image{0, nullptr, 0, 0};
}

// ---- the ring of timing events ----------------------------------------------------------------------------------------------------
// n events per frame for the last `slots` frames (slot = frame % slots).  A step begins its frame with the mask of the events it is to
// record; a record marks its bit only when it succeeded, so timings() never waits on an event that was not recorded.  An event is a
// marker between two launches and costs the stream ~3 us: a loop that is itself being timed records two of them.
struct EventRing {
    int n = 0, slots = 0;           // events per frame; frames in the ring (0: no events)
    int side = -1;                  // the event that may be recorded on another stream than the rest (-1: none)
    hipEvent_t* ev = nullptr;       // slots x n
    long long* frame = nullptr;     // the frame begun in each slot, -1: none (or one stepped with no events)
    unsigned char* want = nullptr;  // the events that frame was to record ...
    unsigned char* mask = nullptr;  // ... and those it did
};

inline void ring_destroy(EventRing& r)
{
    if (r.ev)
        for (int i = 0; i < r.slots * r.n; ++i) if (r.ev[i]) (void)hipEventDestroy(r.ev[i]);
    delete[] r.ev; delete[] r.frame; delete[] r.want; delete[] r.mask;
    r = EventRing{};
}

// (a failed hipEventCreate destroys the events made so far: nothing is left behind)
inline int ring_create(EventRing& r, int n, int slots, int side, const char* what)
{
    r = EventRing{};
    if (!slots) return 0;
    r.n = n; r.slots = slots; r.side = side;
    r.ev = new (std::nothrow) hipEvent_t[(size_t)slots * n]();
    r.frame = new (std::nothrow) long long[slots];
    r.want = new (std::nothrow) unsigned char[slots]();
    r.mask = new (std::nothrow) unsigned char[slots]();
    int e = (r.ev && r.frame && r.want && r.mask) ? 0 : fail_rule(what, KFX_E_RANGE, "out of memory");
    for (int i = 0; !e && i < slots; ++i) r.frame[i] = -1;
    for (int i = 0; !e && i < slots * n; ++i) {   // (hipEventReleaseToDevice events cost the stream the same: measured)
        const hipError_t he = hipEventCreate(&r.ev[i]);
        if (he != hipSuccess) { (void)hipGetLastError(); r.ev[i] = nullptr; e = fail_rule(what, (int)he, "hipEventCreate"); }
    }
    if (e) ring_destroy(r);
    return e;
}

inline void ring_begin(EventRing& r, long long frame, unsigned mask)
{
    if (!r.slots) return;
    const int slot = (int)(frame % r.slots);
    r.frame[slot] = mask ? frame : -1;
    r.want[slot] = (unsigned char)mask;
    r.mask[slot] = 0;
}

// Event k of `frame` on `stream`, if that frame was begun with it and still holds its slot -- also long after the step, as the slab
// frame's side-stream merge needs.  (A failed record leaves an event that timings() would wait on for ever: its bit stays clear.)
inline hipError_t ring_record(EventRing& r, long long frame, int k, hipStream_t stream)
{
    if (!r.slots) return hipSuccess;
    const int slot = (int)(frame % r.slots);
    if (r.frame[slot] != frame || !(r.want[slot] & (1u << k))) return hipSuccess;
    const hipError_t he = hipEventRecord(r.ev[(size_t)slot * r.n + k], stream);
    if (he == hipSuccess) r.mask[slot] |= (unsigned char)(1u << k);
    else (void)hipGetLastError();
    return he;
}

inline unsigned ring_recorded(const EventRing& r, long long frame)
{
    return frame >= 0 && r.frame[frame % r.slots] == frame ? (unsigned)r.mask[frame % r.slots] : 0u;
}
inline hipEvent_t ring_event(const EventRing& r, long long frame, int k) { return r.ev[(size_t)(frame % r.slots) * r.n + k]; }
inline int first_event(unsigned m) { return m ? __builtin_ctz(m) : -1; }
inline int last_event(unsigned m) { return m ? 31 - __builtin_clz(m) : -1; }

// One wait for the latest event any answer about frames [first, last] needs, not for what is queued behind it (events of one stream
// complete in order): the end of the last frame's period -- the next frame's copy of the last frame's first event -- or, failing that,
// the last event of the latest frame that recorded any; then the events of the side stream, which that order does not cover.
inline hipError_t ring_wait(const EventRing& r, long long first, long long last)
{
    hipEvent_t wait_for = nullptr;
    const int b = first_event(ring_recorded(r, last));
    if (b >= 0 && (ring_recorded(r, last + 1) & (1u << b))) wait_for = ring_event(r, last + 1, b);
    for (long long fr = last; !wait_for && fr >= first; --fr)
        if (ring_recorded(r, fr)) wait_for = ring_event(r, fr, last_event(ring_recorded(r, fr)));
    hipError_t he = wait_for ? hipEventSynchronize(wait_for) : hipSuccess;
    for (long long fr = last; r.side >= 0 && he == hipSuccess && fr >= first; --fr)
        if (ring_recorded(r, fr) & (1u << r.side)) he = hipEventSynchronize(ring_event(r, fr, r.side));
    return he;
}

// milliseconds from event a to event b of `frame`; NaN unless it recorded both (or after an error, which stays in he)
inline float ring_span(const EventRing& r, long long frame, int a, int b, hipError_t& he)
{
    float ms = __builtin_nanf("");
    const unsigned m = ring_recorded(r, frame);
    if (he == hipSuccess && a >= 0 && b >= 0 && (m & (1u << a)) && (m & (1u << b))) he = hipEventElapsedTime(&ms, ring_event(r, frame, a), ring_event(r, frame, b));
    return ms;
}
// the frame's first recorded event to the same event of the next frame; NaN unless both recorded it
inline float ring_period(const EventRing& r, long long frame, hipError_t& he)
{
    float ms = __builtin_nanf("");
    const int b = first_event(ring_recorded(r, frame));
    if (he == hipSuccess && b >= 0 && (ring_recorded(r, frame + 1) & (1u << b))) he = hipEventElapsedTime(&ms, ring_event(r, frame, b), ring_event(r, frame + 1, b));
    return ms;
}

// timings() of both frame objects: `fields` floats per frame of [first, first + n) into ms, written by `fill` for a frame that holds
// its slot and all NaN for one stepped with no events; `frames` = steps so far.
inline int ring_timings(const EventRing& r, long long frames, long long first, int n, int fields, float* ms,
                        void (*fill)(const EventRing&, long long frame, float* out, hipError_t& he), const char* what)
{
    if (!r.slots) return fail_rule(what, KFX_E_RANGE, "the frame was created without timing slots");
    if (n <= 0) return 0;
    const long long last = first + n - 1;
    if (first < 0 || last >= frames || frames - first > r.slots) return fail_rule(what, KFX_E_RANGE, "frames not in the ring");
    hipError_t he = ring_wait(r, first, last);
    if (he != hipSuccess) { (void)hipGetLastError(); return fail_rule(what, (int)he, "hipEventSynchronize"); }
    for (int i = 0; i < n; ++i) {
        const long long fr = first + i;
        float* o = ms + (size_t)i * fields;
        for (int k = 0; k < fields; ++k) o[k] = __builtin_nanf("");
        if (r.frame[fr % r.slots] > fr) return fail_rule(what, KFX_E_RANGE, "frame overwritten");
        if (r.frame[fr % r.slots] != fr) continue;   // a frame stepped with no events: NaN
        fill(r, fr, o, he);
        if (he != hipSuccess) { (void)hipGetLastError(); return fail_rule(what, (int)he, "hipEventElapsedTime"); }
    }
    return 0;
}

} // namespace kfx
