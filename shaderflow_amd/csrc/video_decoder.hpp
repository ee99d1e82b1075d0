// video_decoder.hpp — the seam between the video handle (capi_video.hip: slots, copies, events, the matrix) and the compressed source
// formats, a unit each (capi_video_jpeg.hip, capi_video_png.hip). The handle owns one VideoDecoder or none (rgb24 / I420) and knows no
// format: a format's create entry builds its decoder and hands it to video_create; sfx_video_submit_bytes asks it to `accept` the
// pinned frame, a landing frame to `launch`. The decoders' test entries build the same object for one slot.
#pragma once

#include "host_state.hpp"

#include <mutex>

struct VideoDecoder {
    virtual ~VideoDecoder() {}                        // frees the device scratch (the streams that used it have been synchronised)
    virtual const char* name() const = 0;             // for messages: "Motion-JPEG", "PNG"
    // The device scratch: a status word per slot, and one frame's worth of everything else — the decode kernels run in stream order, so one
    // frame's scratch serves all slots. Apart from the constructor, which allocates nothing. false: it could not be allocated.
    virtual bool allocate(int slots) = 0;
    // Why the staged frame of `nbytes` bytes in pinned memory is not one the kernels may be given; null: it is, and what `launch` needs
    // of it is kept for the slot.
    virtual const char* accept(int slot, const void* frame, size_t nbytes) = 0;
    // The decode launches of the slot's frame on `stream`: `staged` (the device's copy of what `accept` saw) → `rgb`; counts the path taken.
    // `first_bad`: pinned words of the handle, {status, serial} of the first bad frame and the format's own behind them, or null.
    virtual void launch(hipStream_t stream, int slot, const uint8_t* staged, uint32_t* first_bad, uint32_t serial, uint8_t* rgb, int bottom_up) = 0;
};

// capi_video.hip: the handle of every create entry — `slots` pinned frames of `frame_bytes` bytes, their device staging, an event each and
// the copy stream. `decoder` (null: rgb24 / I420) is the handle's from here on, on failure too.
int video_create(Context* c, const sfx_handle* boxes, int temporal, int width, int height, int format, size_t frame_bytes, int slots, VideoDecoder* decoder, sfx_handle* out);

// What a format's sfx_video_*_paths entry needs of a handle: its decoder when the handle's source format is `format` (null otherwise),
// the guard under which `launch` runs — the reader thread may submit beside the drawing thread, so a decoder's counters are read under
// it — and the pinned words `launch` was given. false: no video handle.
struct VideoDecoding { VideoDecoder* decoder; std::mutex* guard; Context* ctx; uint32_t* first_bad; };
bool video_decoding(sfx_handle video, int format, VideoDecoding* out);

// What the decoders' test entries share (sfx_jpeg_decode*, sfx_png_decode: one frame outside any handle): device room for the staged frame
// and the pixels, freed on every exit; the frame copied in; the end of the ladder.
struct StagedOnce {
    void *frame = nullptr, *pixels = nullptr;
    ~StagedOnce() { if (frame) hipFree(frame); if (pixels) hipFree(pixels); }
    bool allocate(size_t capacity, size_t pixel_bytes) { return hipMalloc(&frame, capacity) == hipSuccess && hipMalloc(&pixels, pixel_bytes) == hipSuccess; }
    // both zeroed (the pixels' first `rgb_bytes`), then the caller's `nbytes` in front of the frame
    bool copy_in(hipStream_t stream, const void* staged, size_t nbytes, size_t capacity, size_t rgb_bytes) {
        return hipMemsetAsync(frame, 0, capacity, stream) == hipSuccess && hipMemsetAsync(pixels, 0, rgb_bytes, stream) == hipSuccess
               && hipMemcpyAsync(frame, staged, nbytes, hipMemcpyHostToDevice, stream) == hipSuccess;
    }
    // waits for the launches and the read-backs; `ok`: whether all of them were issued. `what` starts the message of a failure.
    int finish(hipStream_t stream, bool ok, const char* what) {
        const hipError_t synced = hipStreamSynchronize(stream);
        return !ok || synced != hipSuccess ? fail(SFX_E_HIP, "%s: %s", what, hipGetErrorString(synced != hipSuccess ? synced : hipGetLastError())) : SFX_OK;
    }
};
