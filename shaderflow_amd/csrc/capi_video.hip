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
//
// Compressed sources: the handle owns a decoder (video_decoder.hpp; a unit per format) and knows nothing else of the format. A slot then
// holds a staged frame of its own length, at most frame_bytes: the submit asks the decoder to accept it, and the landing frame makes the
// decoder's launches where k_video_frame would run.
//
// General planar sources (sfx_video_create_planar: SFX_VIDEO_PLANAR) are uncompressed like rgb24 and I420 — fixed-size slots, no decoder —
// and land through k_video_planar: the handle keeps the kernel's instance and the layout's coefficients, built here on the host.

#include "video_decoder.hpp"
#include "video_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <memory>

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
    std::unique_ptr<VideoDecoder> decoder;  // of a compressed source; null: rgb24 / I420
    void* staging_block = nullptr;          // with a decoder: the slots' device staging as one allocation (`staging` holds views into it)
    uint32_t* first_bad = nullptr;          // with a decoder, pinned: {status, serial} of the first landed frame with a bad status since sfx_video_status last asked (and the decoder's own words: VideoDecoder::launch)
    uint32_t serial = 0;                    // frames landed so far
    int subsampling = 0, sample_bytes = 1, filter = 0;   // SFX_VIDEO_PLANAR: k_video_planar's instance …
    VideoPlanarParams planar = {};                        // … and its coefficients
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
    if (v->staging_block) hipFree(v->staging_block);
    else for (auto p : v->staging) if (p) hipFree(p);
    v->decoder.reset();                                              // (its scratch)
    if (v->first_bad) hipHostFree(v->first_bad);
    if (v->copy) hipStreamDestroy(v->copy);
    v->magic = 0;
    delete v;
}

// With a decoder the staging is one block and the decoder's scratch comes with it. Else every staging frame is an allocation of its own
// with 16 bytes behind it: k_video_frame's 16-byte loads may reach past a frame's last row (video_kernels.hpp).
int video_create(Context* c, const sfx_handle* boxes, int temporal, int width, int height, int format, size_t frame_bytes, int slots, VideoDecoder* decoder, sfx_handle* out) {
    std::unique_ptr<VideoDecoder> owned(decoder);
    const bool staged = decoder != nullptr;
    if (!boxes || !out || temporal < 1 || width < 1 || height < 1 || slots < 1 || slots > 256)
        return fail(SFX_E_INVALID, "video: null boxes or output, or %d x %d, temporal %d, %d slots (1…256)", width, height, temporal, slots);
    USE_DEVICE(c);
    Video* v = new Video();
    v->magic = MAGIC_VIDEO; v->ctx = c; v->temporal = temporal; v->width = width; v->height = height; v->format = format; v->slots = slots;
    v->frame_bytes = frame_bytes; v->decoder = std::move(owned);
    v->boxes.assign(boxes, boxes + temporal);
    for (int d = 0; d < temporal; d++)
        if (!video_texture(v->boxes[d], v)) { delete v; return fail(SFX_E_INVALID, "video: box %d is not a %d x %d RGB8 texture of this context (layers must be 1)", d, width, height); }
    v->host.assign(slots, nullptr); v->staging.assign(slots, nullptr); v->events.assign(slots, nullptr); v->state.assign(slots, SLOT_NEW);
    bool ok = hipStreamCreateWithFlags(&v->copy, hipStreamNonBlocking) == hipSuccess;
    if (ok && staged) ok = hipMalloc(&v->staging_block, frame_bytes*slots) == hipSuccess && hipHostMalloc((void**)&v->first_bad, 64, hipHostMallocDefault) == hipSuccess;
    if (ok && staged) ok = v->decoder->allocate(slots);
    for (int k = 0; ok && k < slots; k++) {
        if (staged) v->staging[k] = (char*)v->staging_block + (size_t)k*frame_bytes;
        else ok = hipMalloc(&v->staging[k], frame_bytes + 16) == hipSuccess;
        ok = ok && hipHostMalloc(&v->host[k], frame_bytes, hipHostMallocDefault) == hipSuccess && hipEventCreateWithFlags(&v->events[k], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        video_release(v);
        return fail(SFX_E_HIP, "video: %d staging frames of %zu bytes (pinned and device)%s could not be allocated", slots, frame_bytes, staged ? " and the decoder's scratch" : "");
    }
    if (v->first_bad) memset(v->first_bad, 0, 64);
    *out = handle_of(v);
    return SFX_OK;
}

bool video_decoding(sfx_handle h, int format, VideoDecoding* out) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v) return false;
    *out = {v->format == format ? v->decoder.get() : nullptr, &v->guard, v->ctx, v->first_bad};
    return true;
}

extern "C" int sfx_video_create(sfx_handle hc, const sfx_handle* boxes, int temporal, int width, int height, int format, int slots, sfx_handle* out) {
    CTX_OR_FAIL(c, hc);
    if (format != SFX_VIDEO_RGB24 && format != SFX_VIDEO_I420) return fail(SFX_E_INVALID, "video: source format %d", format);
    if (format == SFX_VIDEO_I420 && ((width & 1) || (height & 1))) return fail(SFX_E_INVALID, "video: a 4:2:0 source needs even extents, not %d x %d", width, height);
    return video_create(c, boxes, temporal, width, height, format, (size_t)width*height*3/(format == SFX_VIDEO_I420 ? 2 : 1), slots, nullptr, out);   // (extents below 1 are refused there)
}

// The five fixed-point coefficients, the luma offset and the chroma midpoint of a layout (video_kernels.hpp's rule; tests/planar_ref.py
// restates it): floor(x 2^S + 1/2) of ys, 2(1-Kr) cs, 2(1-Kb) Kb/Kg cs, 2(1-Kr) Kr/Kg cs, 2(1-Kb) cs
static VideoPlanarParams planar_coefficients(const sfx_planar_layout& l) {
    static const double KR[3] = {0.299, 0.2126, 0.2627}, KB[3] = {0.114, 0.0722, 0.0593};
    const double kr = KR[l.matrix], kb = KB[l.matrix], kg = 1.0 - kr - kb;
    const int b = l.depth, S = b == 8 ? 8 : (b == 10 ? 14 : 16);
    const double steps = (double)(1 << (b - 8)), top = (double)((1 << b) - 1);
    const double ys = l.range == SFX_PLANAR_FULL ? 255.0/top : 255.0/(219.0*steps), cs = l.range == SFX_PLANAR_FULL ? 255.0/top : 255.0/(224.0*steps);
    const double one = (double)(1 << S);
    auto fixed = [&](double x) { return (int)floor(x*one + 0.5); };
    VideoPlanarParams q;
    q.cy = fixed(ys); q.crv = fixed(2.0*(1.0 - kr)*cs); q.cgu = fixed(2.0*(1.0 - kb)*kb/kg*cs); q.cgv = fixed(2.0*(1.0 - kr)*kr/kg*cs); q.cbu = fixed(2.0*(1.0 - kb)*cs);
    q.offset = l.range == SFX_PLANAR_FULL ? 0 : 16 << (b - 8); q.mid = 1 << (b - 1); q.shift = S; q.depth = b; q.siting = l.siting;
    return q;
}

extern "C" int sfx_video_create_planar(sfx_handle hc, const sfx_handle* boxes, int temporal, int width, int height, const sfx_planar_layout* layout, int slots, sfx_handle* out) {
    CTX_OR_FAIL(c, hc);
    if (!layout) return fail(SFX_E_INVALID, "video: null planar layout");
    const sfx_planar_layout l = *layout;
    if (l.subsampling < SFX_PLANAR_420 || l.subsampling > SFX_PLANAR_MONO) return fail(SFX_E_INVALID, "video: planar layout field subsampling = %d (0 … 3)", l.subsampling);
    if (l.depth != 8 && l.depth != 10 && l.depth != 12) return fail(SFX_E_INVALID, "video: planar layout field depth = %d (8, 10 or 12)", l.depth);
    if (l.subsampling == SFX_PLANAR_MONO && l.depth != 8) return fail(SFX_E_INVALID, "video: planar layout field depth = %d: grey frames are read at 8 bits only", l.depth);
    if (l.matrix < SFX_PLANAR_BT601 || l.matrix > SFX_PLANAR_BT2020) return fail(SFX_E_INVALID, "video: planar layout field matrix = %d (0 … 2)", l.matrix);
    if (l.range != SFX_PLANAR_LIMITED && l.range != SFX_PLANAR_FULL) return fail(SFX_E_INVALID, "video: planar layout field range = %d (0 or 1)", l.range);
    if (l.filter != SFX_PLANAR_NEAREST && l.filter != SFX_PLANAR_LINEAR) return fail(SFX_E_INVALID, "video: planar layout field filter = %d (0 or 1)", l.filter);
    if (l.siting != SFX_PLANAR_CENTRE && l.siting != SFX_PLANAR_LEFT) return fail(SFX_E_INVALID, "video: planar layout field siting = %d (0 or 1)", l.siting);
    if (width < 1 || height < 1) return fail(SFX_E_INVALID, "video: a planar source of %d x %d", width, height);
    const bool halved_x = l.subsampling == SFX_PLANAR_420 || l.subsampling == SFX_PLANAR_422, halved_y = l.subsampling == SFX_PLANAR_420;
    if ((halved_x && (width & 1)) || (halved_y && (height & 1)))
        return fail(SFX_E_INVALID, "video: a %s source needs an even %s, not %d x %d", halved_y ? "4:2:0" : "4:2:2", halved_y ? "width and height" : "width", width, height);
    const size_t bytes = l.depth > 8 ? 2 : 1, luma = (size_t)width*height;
    const size_t chroma = l.subsampling == SFX_PLANAR_MONO ? 0 : (size_t)(halved_x ? width/2 : width)*(halved_y ? height/2 : height);
    const int rc = video_create(c, boxes, temporal, width, height, SFX_VIDEO_PLANAR, (luma + 2*chroma)*bytes, slots, nullptr, out);
    if (rc) return rc;
    Video* v = get<Video>(*out, MAGIC_VIDEO);
    v->subsampling = l.subsampling; v->sample_bytes = (int)bytes;
    v->filter = halved_x ? l.filter : SFX_PLANAR_NEAREST;             // (4:4:4 and grey have nothing to interpolate)
    v->planar = planar_coefficients(l);
    return SFX_OK;
}

// k_video_planar's instance for a handle's layout
template <int SUB, int BPS, int FILTER>
static void planar_launch(const Video* v, dim3 grid, dim3 block, const uint8_t* src, uint8_t* dst) {
    hipLaunchKernelGGL((k_video_planar<SUB, BPS, FILTER>), grid, block, 0, v->ctx->stream, src, dst, v->width, v->height, v->planar);
}
template <int SUB> static void planar_launch_sub(const Video* v, dim3 grid, dim3 block, const uint8_t* src, uint8_t* dst) {
    constexpr bool FILTERED = SUB == PLANAR_420 || SUB == PLANAR_422;
    if (v->sample_bytes == 1) { if (FILTERED && v->filter) planar_launch<SUB, 1, FILTERED ? 1 : 0>(v, grid, block, src, dst); else planar_launch<SUB, 1, 0>(v, grid, block, src, dst); }
    else if constexpr (SUB != PLANAR_MONO) { if (FILTERED && v->filter) planar_launch<SUB, 2, FILTERED ? 1 : 0>(v, grid, block, src, dst); else planar_launch<SUB, 2, 0>(v, grid, block, src, dst); }
}
static void video_launch_planar(const Video* v, const uint8_t* src, uint8_t* dst) {
    const long lanes = video_planar_lanes(v->subsampling, v->width, v->height);
    const dim3 grid((unsigned)((lanes + VIDEO_THREADS - 1)/VIDEO_THREADS)), block(VIDEO_THREADS);
    switch (v->subsampling) {
        case PLANAR_420: planar_launch_sub<PLANAR_420>(v, grid, block, src, dst); break;
        case PLANAR_422: planar_launch_sub<PLANAR_422>(v, grid, block, src, dst); break;
        case PLANAR_444: planar_launch_sub<PLANAR_444>(v, grid, block, src, dst); break;
        default: planar_launch_sub<PLANAR_MONO>(v, grid, block, src, dst); break;
    }
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

// With a decoder the frame's length is its own: the decoder checks the frame, and keeps what its launches need of it, once the slot is known to be the host's
static int video_submit(Video* v, int slot, size_t nbytes) {
    std::lock_guard<std::mutex> lock(v->guard);
    if (v->state[slot] == SLOT_SUBMITTED) return fail(SFX_E_INVALID, "video: slot %d holds a submitted frame that was not consumed yet", slot);
    if (v->decoder) {
        if (const char* fault = v->decoder->accept(slot, v->host[slot], nbytes)) return fail(SFX_E_INVALID, "video: the staged %s frame of %zu bytes in slot %d: %s", v->decoder->name(), nbytes, slot, fault);
        nbytes = (nbytes + 15) & ~(size_t)15;
    }
    USE_DEVICE(v->ctx);
    if (v->state[slot] == SLOT_CONSUMED) HIP_TRY(hipStreamWaitEvent(v->copy, v->events[slot], 0));      // the staging frame is still the last kernel's
    HIP_TRY(hipMemcpyAsync(v->staging[slot], v->host[slot], nbytes, hipMemcpyHostToDevice, v->copy));
    HIP_TRY(hipEventRecord(v->events[slot], v->copy));
    v->state[slot] = SLOT_SUBMITTED;
    return SFX_OK;
}

extern "C" int sfx_video_submit(sfx_handle h, int slot) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v || slot < 0 || slot >= v->slots) return fail(SFX_E_INVALID, "invalid video handle or slot %d", slot);
    if (v->decoder) return fail(SFX_E_INVALID, "video: a %s frame has a length of its own: sfx_video_submit_bytes", v->decoder->name());
    return video_submit(v, slot, v->frame_bytes);
}

extern "C" int sfx_video_submit_bytes(sfx_handle h, int slot, size_t nbytes) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v || slot < 0 || slot >= v->slots) return fail(SFX_E_INVALID, "invalid video handle or slot %d", slot);
    if (!v->decoder && nbytes != v->frame_bytes) return fail(SFX_E_INVALID, "video: a frame of this format has %zu bytes, not %zu", v->frame_bytes, nbytes);
    return video_submit(v, slot, nbytes);
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
    if (v->decoder) v->decoder->launch(v->ctx->stream, slot, (const uint8_t*)v->staging[slot], v->first_bad, v->serial++, (uint8_t*)front->data, 1);
    else if (v->format == SFX_VIDEO_PLANAR) video_launch_planar(v, (const uint8_t*)v->staging[slot], (uint8_t*)front->data);
    else if (v->format == SFX_VIDEO_I420) hipLaunchKernelGGL(k_video_frame<SFX_VIDEO_I420>, grid, block, 0, v->ctx->stream, (const uint8_t*)v->staging[slot], (uint8_t*)front->data, v->width, v->height);
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

// The first bad frame of a compressed source since the last call
extern "C" int sfx_video_status(sfx_handle h, int wait, int64_t* frame, uint32_t* status) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v || !frame || !status) return fail(SFX_E_INVALID, "invalid video handle or null pointer");
    *frame = -1; *status = 0;
    if (!v->decoder) return SFX_OK;                                  // (uncompressed frames have nothing to go wrong)
    volatile uint32_t* note = v->first_bad;
    if (!wait && note[0] == 0u) return SFX_OK;
    USE_DEVICE(v->ctx);
    HIP_TRY(hipStreamSynchronize(v->ctx->stream));
    if (note[0] != 0u) { *status = note[0]; *frame = (int64_t)note[1]; note[1] = 0u; note[0] = 0u; }
    return SFX_OK;
}
