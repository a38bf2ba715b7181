// sensor.hip -- kfx_depth_input (include/kfx_sensor.h): the upload ring in front of the frame.  Host code only: the copy is
// hipMemcpy2DAsync on the ring's own stream, the kernel is kfx_bilateral_depth's (preprocess.hip).
//
// Event protocol, per slot, use j of the slot being image number j * slots + slot:
//   submit(j)  copy stream:  wait consumed(j-1) | copy host -> staging | record uploaded(j)
//   filter(j)  caller's stream: wait uploaded(j) | kernel reads staging | record consumed(j)
//   acquire(j) host: pending < slots (so filter(j-1) was issued and consumed(j-1) recorded), then synchronise uploaded(j-1)
// Every wait follows its record in program order; `up` / `used` say which events were ever recorded, so none is waited on that was not.
#include <new>

#include "kfx_device.h"
#include "host_args.h"
#include "sensor_host.h"

constexpr int KFX_DEPTH_INPUT_MAX_SLOTS = 8;

struct kfx_depth_input {
    size_t w, h, elem;
    int format, slots;
    float s, offset;
    hipStream_t copy;
    void* host[KFX_DEPTH_INPUT_MAX_SLOTS];
    kfx_image staging[KFX_DEPTH_INPUT_MAX_SLOTS];
    hipEvent_t uploaded[KFX_DEPTH_INPUT_MAX_SLOTS], consumed[KFX_DEPTH_INPUT_MAX_SLOTS];
    bool up[KFX_DEPTH_INPUT_MAX_SLOTS], used[KFX_DEPTH_INPUT_MAX_SLOTS];   // uploaded / consumed was recorded at least once
    long long submitted, filtered;   // images submitted / consumed so far: pending = submitted - filtered
    bool held;                       // the buffer of slot submitted % slots is with the caller
};

using namespace kfx;

static void depth_input_free(kfx_depth_input* in)
{
    for (int i = 0; i < in->slots; ++i) {
        if (in->uploaded[i]) (void)hipEventDestroy(in->uploaded[i]);
        if (in->consumed[i]) (void)hipEventDestroy(in->consumed[i]);
        if (in->staging[i].ptr) (void)hipFree(in->staging[i].ptr);
        if (in->host[i]) (void)hipHostFree(in->host[i]);
    }
    if (in->copy) (void)hipStreamDestroy(in->copy);
    (void)hipGetLastError();
    delete in;
}

extern "C" int kfx_depth_input_create(kfx_depth_input** out, size_t w, size_t h, int format, float s, float offset, int slots)
{
    if (!out) return set_error(KFX_E_NULL, "kfx_depth_input_create: null argument");
    *out = nullptr;
    if (format != KFX_DEPTH_U16 && format != KFX_DEPTH_F32) return set_error(KFX_E_RANGE, "kfx_depth_input_create: format is KFX_DEPTH_U16 or KFX_DEPTH_F32");
    if (slots < 2 || slots > KFX_DEPTH_INPUT_MAX_SLOTS) return set_error(KFX_E_RANGE, "kfx_depth_input_create: 2 to 8 slots");
    if (w == 0 || h == 0 || w > (1u << 30) || h > (1u << 30)) return set_error(KFX_E_SHAPE, "kfx_depth_input_create: image dimensions");
    kfx_depth_input* in = new (std::nothrow) kfx_depth_input();   // (value-initialised: every handle null)
    if (!in) return set_error(KFX_E_RANGE, "kfx_depth_input_create: out of memory");
    in->w = w; in->h = h; in->elem = format == KFX_DEPTH_U16 ? 2 : 4;
    in->format = format; in->slots = slots; in->s = s; in->offset = offset;
    const size_t pitch = (w * in->elem + 255) & ~(size_t)255;   // (kfx_alloc_pitched's policy)
    hipError_t he = hipStreamCreateWithFlags(&in->copy, hipStreamNonBlocking);
    const char* what = "kfx_depth_input_create: hipStreamCreateWithFlags";
    if (he != hipSuccess) in->copy = nullptr;
    for (int i = 0; he == hipSuccess && i < slots; ++i) {
        what = "kfx_depth_input_create: hipHostMalloc";
        he = hipHostMalloc(&in->host[i], w * in->elem * h, hipHostMallocDefault);
        if (he != hipSuccess) { in->host[i] = nullptr; break; }
        what = "kfx_depth_input_create: hipMalloc";
        void* d = nullptr;
        he = hipMalloc(&d, pitch * h);
        if (he != hipSuccess) break;
        in->staging[i] = kfx_image{pitch, d, w, h};
        what = "kfx_depth_input_create: hipEventCreate";
        he = hipEventCreateWithFlags(&in->uploaded[i], hipEventDisableTiming);
        if (he != hipSuccess) { in->uploaded[i] = nullptr; break; }
        he = hipEventCreateWithFlags(&in->consumed[i], hipEventDisableTiming);
        if (he != hipSuccess) { in->consumed[i] = nullptr; break; }
    }
    if (he != hipSuccess) {
        (void)hipGetLastError();
        depth_input_free(in);
        return set_error((int)he, what);
    }
    *out = in;
    return 0;
}

extern "C" int kfx_depth_input_destroy(kfx_depth_input* in)
{
    if (!in) return set_error(KFX_E_NULL, "kfx_depth_input_destroy: null ring");
    const hipError_t he = hipStreamSynchronize(in->copy);   // no copy of ours is in flight when its buffers go
    (void)hipGetLastError();
    depth_input_free(in);
    return he == hipSuccess ? 0 : set_error((int)he, "kfx_depth_input_destroy: hipStreamSynchronize");
}

extern "C" int kfx_depth_input_pending(const kfx_depth_input* in)
{
    return in ? (int)(in->submitted - in->filtered) : set_error(KFX_E_NULL, "kfx_depth_input_pending: null ring");
}

extern "C" int kfx_depth_input_acquire(kfx_depth_input* in, void** host_ptr, size_t* pitch)
{
    if (!in || !host_ptr || !pitch) return set_error(KFX_E_NULL, "kfx_depth_input_acquire: null argument");
    if (in->submitted - in->filtered >= in->slots) return set_error(KFX_E_RANGE, "kfx_depth_input_acquire: ring full");
    const int slot = (int)(in->submitted % in->slots);
    if (!in->held && in->up[slot]) {   // the slot's earlier copy has left the buffer
        const hipError_t he = hipEventSynchronize(in->uploaded[slot]);
        if (he != hipSuccess) { (void)hipGetLastError(); return set_error((int)he, "kfx_depth_input_acquire: hipEventSynchronize"); }
    }
    in->held = true;
    *host_ptr = in->host[slot];
    *pitch = in->w * in->elem;
    return 0;
}

extern "C" int kfx_depth_input_submit(kfx_depth_input* in)
{
    if (!in) return set_error(KFX_E_NULL, "kfx_depth_input_submit: null ring");
    if (!in->held) return set_error(KFX_E_RANGE, "kfx_depth_input_submit: no acquired buffer");
    const int slot = (int)(in->submitted % in->slots);
    const kfx_image& st = in->staging[slot];
    if (in->used[slot])   // the kernel that read the staging image's previous content
        if (int e = hip_status(hipStreamWaitEvent(in->copy, in->consumed[slot], 0), "kfx_depth_input_submit: hipStreamWaitEvent")) return e;
    if (int e = hip_status(hipMemcpy2DAsync(st.ptr, st.pitch, in->host[slot], in->w * in->elem, in->w * in->elem, in->h, hipMemcpyHostToDevice, in->copy),
                           "kfx_depth_input_submit: hipMemcpy2DAsync")) return e;
    // (from here the copy is enqueued: the buffer is the ring's again whatever the record says)
    in->held = false;
    if (int e = hip_status(hipEventRecord(in->uploaded[slot], in->copy), "kfx_depth_input_submit: hipEventRecord")) {
        // without its event nobody may wait for this copy: drain it here; the image is pending all the same
        (void)hipStreamSynchronize(in->copy);
        (void)hipGetLastError();
        in->up[slot] = false;
        in->submitted += 1;
        return e;
    }
    in->up[slot] = true;
    in->submitted += 1;
    return 0;
}

int kfx::depth_input_wait(kfx_depth_input* in, kfx_stream stream)
{
    if (!in) return set_error(KFX_E_NULL, "kfx_depth_input_filter: null ring");
    if (in->submitted == in->filtered) return set_error(KFX_E_RANGE, "kfx_depth_input_filter: nothing pending");
    const int slot = (int)(in->filtered % in->slots);
    if (!in->up[slot]) return 0;   // (its submit drained the copy itself)
    return hip_status(hipStreamWaitEvent((hipStream_t)stream, in->uploaded[slot], 0), "kfx_depth_input_filter: hipStreamWaitEvent");
}

int kfx::depth_input_consume(kfx_depth_input* in, const kfx_image* filtered, const kfx_image* metres, float gs, float gr, unsigned size, float minval,
                             kfx_stream stream)
{
    if (!in) return set_error(KFX_E_NULL, "kfx_depth_input_filter: null ring");
    if (in->submitted == in->filtered) return set_error(KFX_E_RANGE, "kfx_depth_input_filter: nothing pending");
    const int slot = (int)(in->filtered % in->slots);
    if (int e = bilateral_depth(filtered, metres, &in->staging[slot], in->format, in->s, in->offset, gs, gr, size, minval, true, stream)) return e;
    in->filtered += 1;   // the launch is enqueued: the image is consumed
    if (int e = hip_status(hipEventRecord(in->consumed[slot], (hipStream_t)stream), "kfx_depth_input_filter: hipEventRecord")) {
        // the next copy into this slot could not wait for the kernel: wait for it here instead
        (void)hipStreamSynchronize((hipStream_t)stream);
        (void)hipGetLastError();
        in->used[slot] = false;
        return e;
    }
    in->used[slot] = true;
    return 0;
}

bool kfx::depth_input_matches(const kfx_depth_input* in, size_t w, size_t h) { return in->w == w && in->h == h; }

extern "C" int kfx_depth_input_filter(kfx_depth_input* in, const kfx_image* filtered, const kfx_image* metres, float gs, float gr, unsigned size,
                                      float minval, kfx_stream stream)
{
    if (!in) return set_error(KFX_E_NULL, "kfx_depth_input_filter: null ring");
    if (in->submitted == in->filtered) return set_error(KFX_E_RANGE, "kfx_depth_input_filter: nothing pending");
    // refused images leave the image pending and the stream untouched
    if (int e = bilateral_depth(filtered, metres, &in->staging[in->filtered % in->slots], in->format, in->s, in->offset, gs, gr, size, minval, false, stream)) return e;
    if (int e = depth_input_wait(in, stream)) return e;
    return depth_input_consume(in, filtered, metres, gs, gr, size, minval, stream);
}
