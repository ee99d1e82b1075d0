// capi_video_png.hip — the PNG decoder of a video handle (video_decoder.hpp; the kernels: png_decode_kernels.hpp): what a
// staged frame must look like, the decoder's device scratch, which inflate path a frame takes and the decode launches — and the entries
// that are PNG's alone: sfx_video_create_png, sfx_video_png_paths and the test entry sfx_png_decode.

#include "video_decoder.hpp"
#include "png_decode_kernels.hpp"

#include <algorithm>
#include <cstdlib>

using namespace sf;

static int png_geometry(int width, int height, size_t capacity) {
    if (width < 1 || height < 1 || (unsigned long long)height*(1ull + 3ull*(unsigned long long)width) > PNG_MAX_OUTPUT)
        return fail(SFX_E_INVALID, "png decode: %d x %d (extents from 1, height x (1 + 3 width) below 2^31)", width, height);
    if (capacity < (size_t)PNG_FRAME_FIXED + 16 || capacity > ((size_t)1 << 30)) return fail(SFX_E_INVALID, "png decode: a staged frame of at most %zu bytes (%d … 2^30)", capacity, PNG_FRAME_FIXED + 16);
    return SFX_OK;
}

// [status words][control: 64 bytes][records: one per segment a staged frame of `capacity` bytes can name, 65 536 at the most][the inflated stream + 64], each part 256-byte aligned
static int png_scratch(int width, int height, size_t capacity, int slots, void** block, uint32_t** status, PngScratch* out) {
    const size_t expected = (size_t)height*(1 + 3*(size_t)width), status_bytes = ((size_t)slots*4 + 255) & ~(size_t)255;
    const size_t records = std::min(capacity/4 + 1, (size_t)65536), record_bytes = (records*sizeof(PngSegmentRecord) + 255) & ~(size_t)255;
    const size_t total = status_bytes + 256 + record_bytes + expected + 64;
    if (hipMalloc(block, total) != hipSuccess) { (void)hipGetLastError(); *block = nullptr; return SFX_E_HIP; }
    if (hipMemset(*block, 0, total) != hipSuccess) { (void)hipGetLastError(); hipFree(*block); *block = nullptr; return SFX_E_HIP; }
    char* base = (char*)*block;
    *status = (uint32_t*)base;
    out->control = (uint32_t*)(base + status_bytes); out->records = (PngSegmentRecord*)(base + status_bytes + 256); out->capacity = (uint32_t)records;
    out->filtered = (uint8_t*)(base + status_bytes + 256 + record_bytes);
    return SFX_OK;
}

// why a staged PNG frame of `nbytes` bytes is not one the kernels may be given (null: it is)
static const char* png_frame_fault(const void* frame, size_t nbytes, int width, int height, size_t capacity, sfx_png_frame* out) {
    if (nbytes < sizeof(sfx_png_frame) || nbytes > capacity) return "its length is outside the record … the slot's capacity";
    sfx_png_frame f;
    memcpy(&f, frame, sizeof f);
    if (f.magic != SFX_PNG_FRAME_MAGIC) return "no SFPN magic";
    if (f.width != (uint32_t)width || f.height != (uint32_t)height) return "another width or height than the video's";
    if (f.segments < 1 || f.payload_offset < sizeof f || (f.payload_offset & 15u) || f.payload_offset > nbytes || f.segments > (f.payload_offset - sizeof f)/4)
        return "the segment table does not lie behind the record and in front of the payload";
    if (f.payload_bytes > nbytes - f.payload_offset) return "the payload does not lie inside the frame";
    uint32_t before = 0;
    for (uint32_t k = 0; k < f.segments; k++) {
        uint32_t start;
        memcpy(&start, (const char*)frame + sizeof f + 4*(size_t)k, 4);
        if ((k == 0 && start != 0) || start < before || start > f.payload_bytes) return "the segment table does not ascend from 0 inside the payload";
        before = start;
    }
    *out = f;
    return nullptr;
}

// Which path a frame takes: SHADERFLOW_PNG_SEGMENTS=0 / 1 force the serial / the segment path; else the segment path when the frame
// has at least two segments and every one but the last ends in 00 00 FF FF (an empty stored block: a flush point). The segment path
// needs a record per segment. (Read per frame: tests switch it.)
static bool png_segments_chosen(const void* frame, const sfx_png_frame& f, uint32_t records, int mode = -1) {
    if (f.segments > records) return false;
    const char* forced = getenv("SHADERFLOW_PNG_SEGMENTS");
    if (mode < 0 && forced && !forced[1] && (forced[0] == '0' || forced[0] == '1')) mode = forced[0] - '0';
    if (mode >= 0) return mode == 1;
    if (f.segments < 2) return false;
    const uint8_t* payload = (const uint8_t*)frame + f.payload_offset;
    static const uint8_t flush[4] = {0x00, 0x00, 0xff, 0xff};
    for (uint32_t k = 1; k < f.segments; k++) {
        uint32_t end;
        memcpy(&end, (const char*)frame + sizeof f + 4*(size_t)k, 4);
        if (end < 4 || memcmp(payload + end - 4, flush, 4)) return false;
    }
    return true;
}

// The decode launches of one staged frame of `nbytes` bytes on `stream` → `rgb`. `status`: the frame's word, cleared in front of them.
// The launch sizes follow from the words sfx_video_submit_bytes validated; the launches run in stream order, so one frame's scratch serves every frame.
static void png_launch_decode(hipStream_t stream, const uint8_t* frame, uint32_t nbytes, uint32_t segments, bool segment_path, const PngScratch& scratch, uint32_t* status,
                              uint32_t* first_bad, uint32_t serial, uint8_t* rgb, int width, int height, int bottom_up) {
    const uint32_t expected = (uint32_t)height*(1u + 3u*(uint32_t)width);
    hipMemsetAsync(status, 0, sizeof(uint32_t), stream);
    hipMemsetAsync(scratch.control, 0, 64, stream);
    if (segment_path) {
        hipLaunchKernelGGL(k_png_inflate_count, dim3(segments), dim3(64), 0, stream, frame, scratch, width, height, nbytes, expected);
        hipLaunchKernelGGL(k_png_inflate_scan, dim3(1), dim3(64), 0, stream, scratch, segments, expected, (volatile uint32_t*)(first_bad ? first_bad + 4 : nullptr));
        hipLaunchKernelGGL(k_png_inflate_write, dim3(segments), dim3(64), 0, stream, frame, scratch);
    }
    hipLaunchKernelGGL(k_png_inflate_serial, dim3(1), dim3(64), 0, stream, frame, scratch, status, width, height, nbytes, expected);
    const unsigned pieces = PNG_ADLER_THREADS*PNG_ADLER_PIECES*16;
    hipLaunchKernelGGL(k_png_adler, dim3((expected + pieces - 1)/pieces), dim3(PNG_ADLER_THREADS), 0, stream, scratch, (const uint32_t*)status, expected);
    hipLaunchKernelGGL(k_png_check, dim3(1), dim3(256), 0, stream, frame, scratch, status, (volatile uint32_t*)first_bad, serial, width, height, expected);
    hipLaunchKernelGGL(k_png_unfilter, dim3(1), dim3(PNG_UNFILTER_WAVES*64), 0, stream, (const uint8_t*)scratch.filtered, rgb, (const uint32_t*)status, width, height, bottom_up);
}

// Every slot holds a staged frame of its own length, at most `capacity` bytes. `mode` is the test entry's knob (png_segments_chosen).
struct PngDecoder : VideoDecoder {
    const int width, height, mode;
    const size_t capacity;
    void* block = nullptr;                          // [status: a word per slot][control][segment records][the inflated stream]
    uint32_t* status = nullptr;
    PngScratch scratch{};
    std::vector<uint32_t> staged_bytes, segments;   // of the frame each slot holds
    std::vector<uint8_t> segment_path;              // whether that frame takes the segment path (chosen when it is accepted)
    uint64_t serial_frames = 0;                     // landed frames that took the serial path up front (the others count themselves: first_bad[4], [5])

    PngDecoder(int width, int height, size_t capacity, int mode = -1) : width(width), height(height), mode(mode), capacity(capacity) {}
    ~PngDecoder() override { if (block) hipFree(block); }
    const char* name() const override { return "PNG"; }
    bool allocate(int slots) override {
        staged_bytes.assign(slots, 0); segments.assign(slots, 0); segment_path.assign(slots, 0);
        return png_scratch(width, height, capacity, slots, &block, &status, &scratch) == SFX_OK;
    }
    const char* accept(int slot, const void* frame, size_t nbytes) override {
        sfx_png_frame f;
        if (const char* fault = png_frame_fault(frame, nbytes, width, height, capacity, &f)) return fault;
        staged_bytes[slot] = (uint32_t)nbytes; segments[slot] = f.segments;
        segment_path[slot] = png_segments_chosen(frame, f, scratch.capacity, mode) ? 1 : 0;
        return nullptr;
    }
    void launch(hipStream_t stream, int slot, const uint8_t* staged, uint32_t* first_bad, uint32_t serial, uint8_t* rgb, int bottom_up) override {
        if (!segment_path[slot]) serial_frames++;
        png_launch_decode(stream, staged, staged_bytes[slot], segments[slot], segment_path[slot] != 0, scratch, status + slot, first_bad, serial, rgb, width, height, bottom_up);
    }
};

extern "C" int sfx_video_create_png(sfx_handle hc, const sfx_handle* boxes, int temporal, int width, int height, size_t capacity, int slots, sfx_handle* out) {
    CTX_OR_FAIL(c, hc);
    if (const int rc = png_geometry(width, height, capacity)) return rc;
    capacity = (capacity + 15) & ~(size_t)15;
    return video_create(c, boxes, temporal, width, height, SFX_VIDEO_PNG, capacity, slots, new PngDecoder(width, height, capacity), out);
}

extern "C" int sfx_video_png_paths(sfx_handle h, uint64_t* segment_frames, uint64_t* serial_frames) {
    VideoDecoding v;
    if (!segment_frames || !serial_frames || !video_decoding(h, SFX_VIDEO_PNG, &v)) return fail(SFX_E_INVALID, "invalid video handle or null pointer");
    *segment_frames = *serial_frames = 0;
    if (!v.decoder) return SFX_OK;
    USE_DEVICE(v.ctx);
    HIP_TRY(hipStreamSynchronize(v.ctx->stream));                    // (the scan kernel of a frame says which way it went)
    std::lock_guard<std::mutex> lock(*v.guard);
    volatile uint32_t* counted = v.first_bad + 4;
    *segment_frames = counted[0]; *serial_frames = static_cast<const PngDecoder*>(v.decoder)->serial_frames + counted[1];
    return SFX_OK;
}

// The decoder a handle would have, for one slot
extern "C" int sfx_png_decode(sfx_handle hc, const void* staged, size_t nbytes, int width, int height, int mode, uint8_t* filtered_out, uint8_t* rgb_out,
                              uint32_t* status, uint32_t* info) {
    CTX_OR_FAIL(c, hc);
    if (!staged || !status) return fail(SFX_E_INVALID, "png decode: null frame or status");
    if (mode < -1 || mode > 1) return fail(SFX_E_INVALID, "png decode: mode %d (0: serial, 1: segments, -1: as a video handle chooses)", mode);
    const size_t capacity = (std::max(nbytes, (size_t)PNG_FRAME_FIXED + 16) + 15) & ~(size_t)15;
    if (const int rc = png_geometry(width, height, capacity)) return rc;
    if (info) info[0] = info[1] = info[2] = 0u;
    USE_DEVICE(c);
    PngDecoder decoder(width, height, capacity, mode);
    StagedOnce once;
    const size_t rgb_bytes = (size_t)width*height*3, filtered_bytes = (size_t)height*(1 + 3*(size_t)width);
    if (!decoder.allocate(1) || !once.allocate(capacity, rgb_bytes + 64)) {
        (void)hipGetLastError();
        return fail(SFX_E_HIP, "png decode: the scratch of a %d x %d frame could not be allocated", width, height);
    }
    if (const char* fault = decoder.accept(0, staged, nbytes)) return fail(SFX_E_INVALID, "png decode: the staged frame of %zu bytes: %s", nbytes, fault);
    uint8_t* filtered = decoder.scratch.filtered;
    // 64 guard bytes behind the inflated stream and behind the pixels: whatever the stream says, the kernels leave them alone
    bool ok = once.copy_in(c->stream, staged, nbytes, capacity, rgb_bytes) && hipMemsetAsync((char*)once.pixels + rgb_bytes, 0xa5, 64, c->stream) == hipSuccess
              && hipMemsetAsync(filtered + filtered_bytes, 0xa5, 64, c->stream) == hipSuccess;
    if (ok) {
        decoder.launch(c->stream, 0, (const uint8_t*)once.frame, nullptr, 0, (uint8_t*)once.pixels, 0);
        ok = hipGetLastError() == hipSuccess;
    }
    uint32_t control[2] = {0u, 0u};
    uint8_t guards[128];
    if (ok) ok = hipMemcpyAsync(guards, filtered + filtered_bytes, 64, hipMemcpyDeviceToHost, c->stream) == hipSuccess
                 && hipMemcpyAsync(guards + 64, (char*)once.pixels + rgb_bytes, 64, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (ok && filtered_out) ok = hipMemcpyAsync(filtered_out, filtered, filtered_bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (ok && rgb_out) ok = hipMemcpyAsync(rgb_out, once.pixels, rgb_bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (ok) ok = hipMemcpyAsync(status, decoder.status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) == hipSuccess
                 && hipMemcpyAsync(control, decoder.scratch.control, sizeof control, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    const int rc = once.finish(c->stream, ok, "png decode");
    if (rc) return rc;
    if (std::any_of(guards, guards + 128, [](uint8_t v) { return v != 0xa5; })) return fail(SFX_E_HIP, "png decode: the kernels wrote behind the inflated stream or behind the pixels");
    if (info) { info[0] = decoder.segments[0]; info[1] = control[0]; info[2] = decoder.segment_path[0] ? control[1] : 0u; }
    return SFX_OK;
}
