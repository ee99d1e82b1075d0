// capi_video.hip — the C-ABI's video part (include/shaderflow_hip.h: sfx_video_*): source frames of a ShaderVideo staged in pinned host
// memory, copied to device staging on a copy stream of the handle's own, and put into the module's texture matrix by k_video_frame
// (video_kernels.hpp) on the context's render stream. capi.hip's run_sequence launches the same frame in front of the scene frame that
// first shows it (video_launch_frame, host_state.hpp).
//
// A slot's life: sfx_video_slot (the host fills the pinned frame) → sfx_video_submit (host → device on the copy stream, the slot's event
// behind it) → sfx_video_step / a landing frame of sfx_sequence_run (the render stream waits for the event, the matrix rolls,
// k_video_frame writes the front box, the slot's event is recorded again BEHIND the kernel: the slot is free). The next
// sfx_video_slot of that slot waits for the event on the host, the next sfx_video_submit makes the copy stream wait for it, so neither
// the pinned frame nor the device staging is overwritten while something still reads it. One thread may fill and submit slots while
// another draws (videosequence.py's reader): the slots' states are guarded, and a thread only ever touches slots the other has handed over.

#include "host_state.hpp"
#include "video_kernels.hpp"

#include <algorithm>
#include <mutex>

using namespace sf;

struct Video : Object {
    Context* ctx;
    int temporal = 1, width = 0, height = 0, format = 0, slots = 0;
    size_t frame_bytes = 0;
    std::vector<sfx_handle> boxes;          // the matrix' rows in their CURRENT order: boxes[0] is the front
    hipStream_t copy = nullptr;
    std::vector<void*> host, staging;
    std::vector<hipEvent_t> events;
    std::vector<int> state;                 // per slot: SLOT_*
    std::mutex guard;
};
enum { SLOT_NEW = 0, SLOT_SUBMITTED = 1, SLOT_CONSUMED = 2 };

static Texture* video_texture(sfx_handle h, const Video* v) {
    Texture* t = get<Texture>(h, MAGIC_TEX);
    if (!t || t->ctx != v->ctx || t->dtype != SFX_U8 || t->components != 3 || t->width != v->width || t->height != v->height || !t->data) return nullptr;
    return t;
}

static void video_release(Video* v) {
    hipSetDevice(v->ctx->device);
    if (v->copy) hipStreamSynchronize(v->copy);                      // the copy stream stops before its buffers go
    hipStreamSynchronize(v->ctx->stream);
    for (auto e : v->events) if (e) hipEventDestroy(e);
    for (auto p : v->host) if (p) hipHostFree(p);
    for (auto p : v->staging) if (p) hipFree(p);
    if (v->copy) hipStreamDestroy(v->copy);
    v->magic = 0;
    delete v;
}

extern "C" int sfx_video_create(sfx_handle hc, const sfx_handle* boxes, int temporal, int width, int height, int format, int slots, sfx_handle* out) {
    CTX_OR_FAIL(c, hc);
    if (!boxes || !out || temporal < 1 || width < 1 || height < 1 || slots < 1 || slots > 256) return fail(SFX_E_INVALID, "video: null boxes or output, or %d x %d, temporal %d, %d slots", width, height, temporal, slots);
    if (format != SFX_VIDEO_RGB24 && format != SFX_VIDEO_I420) return fail(SFX_E_INVALID, "video: source format %d", format);
    if (format == SFX_VIDEO_I420 && ((width & 1) || (height & 1))) return fail(SFX_E_INVALID, "video: a 4:2:0 source needs even extents, not %d x %d", width, height);
    USE_DEVICE(c);
    Video* v = new Video();
    v->magic = MAGIC_VIDEO; v->ctx = c; v->temporal = temporal; v->width = width; v->height = height; v->format = format; v->slots = slots;
    v->frame_bytes = format == SFX_VIDEO_I420 ? (size_t)width*height*3/2 : (size_t)width*height*3;
    v->boxes.assign(boxes, boxes + temporal);
    for (int d = 0; d < temporal; d++)
        if (!video_texture(v->boxes[d], v)) { delete v; return fail(SFX_E_INVALID, "video: box %d is not a %d x %d RGB8 texture of this context (layers must be 1)", d, width, height); }
    v->host.assign(slots, nullptr); v->staging.assign(slots, nullptr); v->events.assign(slots, nullptr); v->state.assign(slots, SLOT_NEW);
    bool ok = hipStreamCreateWithFlags(&v->copy, hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; ok && k < slots; k++)
        ok = hipHostMalloc(&v->host[k], v->frame_bytes, hipHostMallocDefault) == hipSuccess && hipMalloc(&v->staging[k], v->frame_bytes + 16) == hipSuccess
             && hipEventCreateWithFlags(&v->events[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        const size_t frame_bytes = v->frame_bytes;
        (void)hipGetLastError();
        video_release(v);
        return fail(SFX_E_HIP, "video: %d staging frames of %zu bytes (pinned and device) could not be allocated", slots, frame_bytes);
    }
    *out = handle_of(v);
    return SFX_OK;
}

extern "C" int sfx_video_slot(sfx_handle h, int slot, void** host, size_t* nbytes) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v || slot < 0 || slot >= v->slots) return fail(SFX_E_INVALID, "invalid video handle or slot %d", slot);
    int state;
    { std::lock_guard<std::mutex> lock(v->guard); state = v->state[slot]; }
    if (state == SLOT_SUBMITTED) return fail(SFX_E_INVALID, "video: slot %d holds a submitted frame that was not consumed yet", slot);
    if (state == SLOT_CONSUMED) {                                    // the kernel that read the slot's frame has run: the pinned frame is the host's again
        USE_DEVICE(v->ctx);
        HIP_TRY(hipEventSynchronize(v->events[slot]));
    }
    if (host) *host = v->host[slot];
    if (nbytes) *nbytes = v->frame_bytes;
    return SFX_OK;
}

extern "C" int sfx_video_submit(sfx_handle h, int slot) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v || slot < 0 || slot >= v->slots) return fail(SFX_E_INVALID, "invalid video handle or slot %d", slot);
    std::lock_guard<std::mutex> lock(v->guard);
    if (v->state[slot] == SLOT_SUBMITTED) return fail(SFX_E_INVALID, "video: slot %d holds a submitted frame that was not consumed yet", slot);
    USE_DEVICE(v->ctx);
    if (v->state[slot] == SLOT_CONSUMED) HIP_TRY(hipStreamWaitEvent(v->copy, v->events[slot], 0));      // the staging frame is still the last kernel's
    HIP_TRY(hipMemcpyAsync(v->staging[slot], v->host[slot], v->frame_bytes, hipMemcpyHostToDevice, v->copy));
    HIP_TRY(hipEventRecord(v->events[slot], v->copy));
    v->state[slot] = SLOT_SUBMITTED;
    return SFX_OK;
}

// One landing frame on the context's render stream, in stream order with the draws behind it
int video_launch_frame(sfx_handle h, Context* c, int slot) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v) return fail(SFX_E_INVALID, "invalid video handle");
    if (c && v->ctx != c) return fail(SFX_E_INVALID, "video: the handle belongs to another context");
    if (slot < 0 || slot >= v->slots) return fail(SFX_E_INVALID, "video: slot %d of %d", slot, v->slots);
    std::lock_guard<std::mutex> lock(v->guard);
    if (v->state[slot] != SLOT_SUBMITTED) return fail(SFX_E_INVALID, "video: slot %d holds no submitted frame", slot);
    // texture.roll() of video.py:109: the oldest row becomes the front, and is what the frame is written into
    // (the scene may have re-made a texture since sfx_video_create: a stale handle is an error, not a write into freed memory)
    Texture* front = video_texture(v->boxes.back(), v);
    if (!front) return fail(SFX_E_INVALID, "video: a texture of the module was released or re-made after sfx_video_create");
    if (front->nbytes < (size_t)v->width*v->height*3) return fail(SFX_E_INVALID, "video: the texture holds %zu bytes, a frame %zu", front->nbytes, (size_t)v->width*v->height*3);
    HIP_TRY(hipStreamWaitEvent(v->ctx->stream, v->events[slot], 0));
    std::rotate(v->boxes.begin(), v->boxes.end() - 1, v->boxes.end());
    const long lanes = video_frame_lanes(v->format, v->width, v->height);
    const dim3 grid((unsigned)((lanes + VIDEO_THREADS - 1)/VIDEO_THREADS)), block(VIDEO_THREADS);
    if (v->format == SFX_VIDEO_I420) hipLaunchKernelGGL(k_video_frame<SFX_VIDEO_I420>, grid, block, 0, v->ctx->stream, (const uint8_t*)v->staging[slot], (uint8_t*)front->data, v->width, v->height);
    else hipLaunchKernelGGL(k_video_frame<SFX_VIDEO_RGB24>, grid, block, 0, v->ctx->stream, (const uint8_t*)v->staging[slot], (uint8_t*)front->data, v->width, v->height);
    const int rc = launch_status();
    if (rc) return rc;
    HIP_TRY(hipEventRecord(v->events[slot], v->ctx->stream));          // the slot is free behind the kernel
    v->state[slot] = SLOT_CONSUMED;
    return SFX_OK;
}

// the box `depth` frames back in the matrix' current order (0: the front); 0 when there is none
sfx_handle video_box(sfx_handle h, int depth) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    return (v && depth >= 0 && depth < v->temporal) ? v->boxes[depth] : 0;
}
int video_temporal(sfx_handle h, Context* c) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    return (v && v->ctx == c) ? v->temporal : -1;
}

extern "C" int sfx_video_step(sfx_handle h, int slot) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v) return fail(SFX_E_INVALID, "invalid video handle");
    USE_DEVICE(v->ctx);
    return video_launch_frame(h, v->ctx, slot);
}

extern "C" int sfx_video_destroy(sfx_handle h) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v) return fail(SFX_E_INVALID, "invalid video handle");
    video_release(v);
    return SFX_OK;
}
