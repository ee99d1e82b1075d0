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
#include "jpeg_decode_kernels.hpp"
#include "png_decode_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
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
    // SFX_VIDEO_MJPEG: every slot holds a staged frame of its own length (jpeg_decode_kernels.hpp), at most frame_bytes of them
    JpegDecodeGeometry jpeg{};
    std::vector<uint32_t> intervals, scan_bytes;     // restart intervals and scan bytes of the frame each slot holds
    void* sync_block = nullptr;             // the subsequence path's records (jpeg_decode_kernels.hpp, 1b), for capacity/JPEG_SYNC_SUBSEQUENCE lanes and one per interval
    JpegSyncScratch sync{};
    uint32_t sync_bytes = 0;                // a subsequence's bytes on this handle
    uint64_t sync_frames = 0, serial_frames = 0;    // landed frames by entropy path (sfx_video_jpeg_paths)
    void* staging_block = nullptr;          // the slots' device staging as one allocation (`staging` holds views into it)
    void* scratch = nullptr;                // [basis 64 f32][status: a word per slot][coefficients][planes]: the decode kernels run in stream order, one frame's scratch serves all slots
    float* basis = nullptr; uint32_t* status = nullptr; int16_t* coefficients = nullptr; uint8_t* planes = nullptr;
    uint32_t* first_bad = nullptr;          // pinned: {status, serial} of the first landed frame with a bad status since sfx_video_status last asked
    uint32_t serial = 0;                    // frames landed so far
    // SFX_VIDEO_PNG: staged frames as above; `scratch` is [status: a word per slot][control][segment records][the inflated stream]
    PngScratch png{};
    std::vector<uint32_t> staged_bytes, segments;    // of the frame each slot holds
    std::vector<uint8_t> segment_path;               // whether that frame takes the segment path (png_segments_chosen, at submit)
    uint64_t png_serial_frames = 0;                  // landed frames that took the serial path up front (the others count themselves: first_bad[4], [5])
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
    if (v->scratch) hipFree(v->scratch);
    if (v->sync_block) hipFree(v->sync_block);
    if (v->first_bad) hipHostFree(v->first_bad);
    if (v->copy) hipStreamDestroy(v->copy);
    v->magic = 0;
    delete v;
}

static int jpeg_decode_geometry(int width, int height, int components, int hs, int vs, size_t capacity, JpegDecodeGeometry* g) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return fail(SFX_E_INVALID, "jpeg decode: %d x %d (extents 1…65535)", width, height);
    if (components != 1 && components != 3) return fail(SFX_E_INVALID, "jpeg decode: %d components (1: grey, 3: YCbCr)", components);
    if (components == 1) hs = vs = 1;
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return fail(SFX_E_INVALID, "jpeg decode: luma sampling %d x %d (2x2, 2x1 or 1x1)", hs, vs);
    if (capacity < (size_t)JPEG_FRAME_FIXED + 16 || capacity > ((size_t)1 << 30)) return fail(SFX_E_INVALID, "jpeg decode: a staged frame of at most %zu bytes (%d … 2^30)", capacity, JPEG_FRAME_FIXED + 16);
    g->width = width; g->height = height; g->components = components; g->hs = hs; g->vs = vs;
    g->mcus_x = (width + 8*hs - 1)/(8*hs); g->mcus_y = (height + 8*vs - 1)/(8*vs); g->blocks = components == 1 ? 1 : hs*vs + 2;
    g->capacity = (int)((capacity + 15) & ~(size_t)15);
    return SFX_OK;
}

// [basis 64 f32][status words, 64 bytes' worth at least][coefficients][planes], each part 256-byte aligned
static int jpeg_scratch(const JpegDecodeGeometry& g, int slots, void** scratch, float** basis, uint32_t** status, int16_t** coefficients, uint8_t** planes) {
    const size_t status_bytes = ((size_t)slots*4 + 255) & ~(size_t)255, coefficient_bytes = (jpeg_decode_coefficients(g)*2 + 255) & ~(size_t)255;
    if (hipMalloc(scratch, 256 + status_bytes + coefficient_bytes + jpeg_plane_bytes(g)) != hipSuccess) { (void)hipGetLastError(); *scratch = nullptr; return SFX_E_HIP; }
    char* base = (char*)*scratch;
    *basis = (float*)base; *status = (uint32_t*)(base + 256); *coefficients = (int16_t*)(base + 256 + status_bytes); *planes = (uint8_t*)(base + 256 + status_bytes + coefficient_bytes);
    float dct[64];
    jpeg_dct_basis(dct);
    if (hipMemcpy(*basis, dct, sizeof dct, hipMemcpyHostToDevice) != hipSuccess || hipMemset(*status, 0, status_bytes) != hipSuccess) { (void)hipGetLastError(); hipFree(*scratch); *scratch = nullptr; return SFX_E_HIP; }
    return SFX_OK;
}

// The production values of the subsequence path: a subsequence's bytes (64, 128 and 256 were measured, 64 was the fastest on every clip:
// DESIGN.md §7c, profiles/mjpeg_in_bench.txt), the rounds of a phase (the most the two phases allow; rounds end when nothing changes), and
// how many subsequences a frame's mean restart interval must hold at least for the frame to take the path.
enum { JPEG_SYNC_SUBSEQUENCE = 64, JPEG_SYNC_ROUNDS = 255, JPEG_SYNC_RULE = 4 };

// Records for frames of `capacity` bytes cut into pieces of `subsequence` bytes: [records][handoff][rounds: two phases][control: 64 bytes]
static int jpeg_sync_scratch(const JpegDecodeGeometry& g, size_t capacity, uint32_t subsequence, void** block, JpegSyncScratch* out) {
    const size_t mcus = (size_t)g.mcus_x*g.mcus_y;
    const size_t records = capacity/subsequence + 1 + std::min(mcus, capacity/4);      // (an interval costs the frame a table word)
    const size_t workgroups = (records + JPEG_SYNC_LANES - 1)/JPEG_SYNC_LANES;
    if (records > 0xffffffffull) return SFX_E_TOO_LARGE;
    const size_t record_bytes = records*sizeof(JpegSyncRecord), handoff_bytes = workgroups*sizeof(uint2), round_bytes = (2*workgroups*4 + 63) & ~(size_t)63;
    if (hipMalloc(block, record_bytes + handoff_bytes + round_bytes + 64) != hipSuccess) { (void)hipGetLastError(); *block = nullptr; return SFX_E_HIP; }
    if (hipMemset(*block, 0, record_bytes + handoff_bytes + round_bytes + 64) != hipSuccess) { (void)hipGetLastError(); hipFree(*block); *block = nullptr; return SFX_E_HIP; }
    char* base = (char*)*block;
    out->records = (JpegSyncRecord*)base; out->handoff = (uint2*)(base + record_bytes); out->rounds = (uint32_t*)(base + record_bytes + handoff_bytes);
    out->control = (uint32_t*)(base + record_bytes + handoff_bytes + round_bytes); out->capacity = (uint32_t)records;
    return SFX_OK;
}

// A subsequence's bytes for a new handle: the production value, or SHADERFLOW_JPEG_SYNC_BYTES (2 … 2^20; for measurements)
static uint32_t jpeg_sync_bytes() {
    const char* text = getenv("SHADERFLOW_JPEG_SYNC_BYTES");
    const long asked = text ? strtol(text, nullptr, 10) : 0;
    return asked >= 2 && asked <= (1 << 20) ? (uint32_t)asked : (uint32_t)JPEG_SYNC_SUBSEQUENCE;
}

// Which entropy path a frame takes: SHADERFLOW_JPEG_SYNC=0 / 1 force the lane-per-interval kernel / the subsequence path; else the
// subsequence path when the frame's mean restart interval holds JPEG_SYNC_RULE subsequences. (Read per frame: tests switch it.)
static bool jpeg_sync_chosen(uint32_t scan_bytes, uint32_t intervals, uint32_t subsequence) {
    const char* forced = getenv("SHADERFLOW_JPEG_SYNC");
    if (forced && forced[0] == '0' && !forced[1]) return false;
    if (forced && forced[0] == '1' && !forced[1]) return true;
    return intervals > 0 && scan_bytes/intervals >= (unsigned long long)JPEG_SYNC_RULE*subsequence;
}

// ---- PNG (png_decode_kernels.hpp) ------------------------------------------------------------------------------------------------------

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

// The handle of either entry below: `slots` pinned frames of `frame_bytes` bytes, their device staging, an event each and the copy
// stream. `jpeg` (SFX_VIDEO_MJPEG): the staging is one block and the decoder's scratch comes with it. Else every staging frame is an
// allocation of its own with 16 bytes behind it: k_video_frame's 16-byte loads may reach past a frame's last row (video_kernels.hpp).
static int video_create(Context* c, const sfx_handle* boxes, int temporal, int width, int height, int format, size_t frame_bytes, int slots,
                        const JpegDecodeGeometry* jpeg, sfx_handle* out) {
    const bool png = format == SFX_VIDEO_PNG, staged = jpeg || png;
    if (!boxes || !out || temporal < 1 || width < 1 || height < 1 || slots < 1 || slots > 256)
        return fail(SFX_E_INVALID, "video: null boxes or output, or %d x %d, temporal %d, %d slots (1…256)", width, height, temporal, slots);
    USE_DEVICE(c);
    Video* v = new Video();
    v->magic = MAGIC_VIDEO; v->ctx = c; v->temporal = temporal; v->width = width; v->height = height; v->format = format; v->slots = slots;
    v->frame_bytes = frame_bytes;
    if (jpeg) { v->jpeg = *jpeg; v->sync_bytes = jpeg_sync_bytes(); }
    v->boxes.assign(boxes, boxes + temporal);
    for (int d = 0; d < temporal; d++)
        if (!video_texture(v->boxes[d], v)) { delete v; return fail(SFX_E_INVALID, "video: box %d is not a %d x %d RGB8 texture of this context (layers must be 1)", d, width, height); }
    v->host.assign(slots, nullptr); v->staging.assign(slots, nullptr); v->events.assign(slots, nullptr); v->state.assign(slots, SLOT_NEW); v->intervals.assign(slots, 0); v->scan_bytes.assign(slots, 0);
    v->staged_bytes.assign(slots, 0); v->segments.assign(slots, 0); v->segment_path.assign(slots, 0);
    bool ok = hipStreamCreateWithFlags(&v->copy, hipStreamNonBlocking) == hipSuccess;
    if (ok && staged) ok = hipMalloc(&v->staging_block, frame_bytes*slots) == hipSuccess && hipHostMalloc((void**)&v->first_bad, 64, hipHostMallocDefault) == hipSuccess;
    if (ok && png) ok = png_scratch(width, height, frame_bytes, slots, &v->scratch, &v->status, &v->png) == SFX_OK;
    if (ok && jpeg)
        ok = jpeg_scratch(*jpeg, slots, &v->scratch, &v->basis, &v->status, &v->coefficients, &v->planes) == SFX_OK
             && jpeg_sync_scratch(*jpeg, frame_bytes, v->sync_bytes, &v->sync_block, &v->sync) == SFX_OK;
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

extern "C" int sfx_video_create(sfx_handle hc, const sfx_handle* boxes, int temporal, int width, int height, int format, int slots, sfx_handle* out) {
    CTX_OR_FAIL(c, hc);
    if (format != SFX_VIDEO_RGB24 && format != SFX_VIDEO_I420) return fail(SFX_E_INVALID, "video: source format %d", format);
    if (format == SFX_VIDEO_I420 && ((width & 1) || (height & 1))) return fail(SFX_E_INVALID, "video: a 4:2:0 source needs even extents, not %d x %d", width, height);
    return video_create(c, boxes, temporal, width, height, format, (size_t)width*height*3/(format == SFX_VIDEO_I420 ? 2 : 1), slots, nullptr, out);   // (extents below 1 are refused there)
}

extern "C" int sfx_video_create_mjpeg(sfx_handle hc, const sfx_handle* boxes, int temporal, int width, int height, int components, int h_sampling, int v_sampling,
                                      size_t capacity, int slots, sfx_handle* out) {
    CTX_OR_FAIL(c, hc);
    JpegDecodeGeometry g;
    if (const int rc = jpeg_decode_geometry(width, height, components, h_sampling, v_sampling, capacity, &g)) return rc;
    return video_create(c, boxes, temporal, width, height, SFX_VIDEO_MJPEG, (size_t)g.capacity, slots, &g, out);
}

extern "C" int sfx_video_create_png(sfx_handle hc, const sfx_handle* boxes, int temporal, int width, int height, size_t capacity, int slots, sfx_handle* out) {
    CTX_OR_FAIL(c, hc);
    if (const int rc = png_geometry(width, height, capacity)) return rc;
    return video_create(c, boxes, temporal, width, height, SFX_VIDEO_PNG, (capacity + 15) & ~(size_t)15, slots, nullptr, out);
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

// why a staged Motion-JPEG frame of `nbytes` bytes is not one the kernels may be given (null: it is, and `intervals` is its interval count)
static const char* jpeg_frame_fault(const void* frame, size_t nbytes, const JpegDecodeGeometry& g, uint32_t* intervals, uint32_t* scan_bytes) {
    if (nbytes < sizeof(sfx_jpeg_frame) || nbytes > (size_t)g.capacity) return "its length is outside the fixed part … the slot's capacity";
    sfx_jpeg_frame f;
    memcpy(&f, frame, sizeof f);                                     // (sfx_jpeg_decode's caller owes no alignment)
    static const char* const why[] = {nullptr, "no SFJD magic", "the interval count does not follow from the restart interval and the geometry",
                                      "the scan does not lie behind the interval table and inside the frame"};
    if (const int fault = jpeg_descriptor_fault(f, g.mcus_x, g.mcus_y, nbytes)) return why[fault];
    if ((int)f.components != g.components) return "another component count than the video's";
    for (int c = 0; c < g.components; c++)
        if (f.tq[c] > 3 || f.td[c] > 1 || f.ta[c] > 1) return "a table selector outside 0…3 (quantisation) or 0…1 (Huffman)";
    for (const sfx_jpeg_huffman& table : f.huffman) {
        int count = 0;
        for (int k = 0; k < 16; k++) count += table.bits[k];
        if (count > 256) return "a Huffman table with more than 256 codes";
    }
    *intervals = f.intervals;
    *scan_bytes = f.scan_bytes;
    return nullptr;
}

// `staged`: the frame's length is its own (SFX_VIDEO_MJPEG): it is checked, and its interval count kept, once the slot is known to be the host's
static int video_submit(Video* v, int slot, size_t nbytes, bool staged = false) {
    std::lock_guard<std::mutex> lock(v->guard);
    if (v->state[slot] == SLOT_SUBMITTED) return fail(SFX_E_INVALID, "video: slot %d holds a submitted frame that was not consumed yet", slot);
    if (staged && v->format == SFX_VIDEO_PNG) {
        sfx_png_frame f;
        if (const char* fault = png_frame_fault(v->host[slot], nbytes, v->width, v->height, v->frame_bytes, &f)) return fail(SFX_E_INVALID, "video: the staged PNG frame of %zu bytes in slot %d: %s", nbytes, slot, fault);
        v->staged_bytes[slot] = (uint32_t)nbytes; v->segments[slot] = f.segments;
        v->segment_path[slot] = png_segments_chosen(v->host[slot], f, v->png.capacity) ? 1 : 0;
        nbytes = (nbytes + 15) & ~(size_t)15;
    } else if (staged) {
        if (const char* fault = jpeg_frame_fault(v->host[slot], nbytes, v->jpeg, &v->intervals[slot], &v->scan_bytes[slot])) return fail(SFX_E_INVALID, "video: the staged Motion-JPEG frame of %zu bytes in slot %d: %s", nbytes, slot, fault);
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
    if (v->format == SFX_VIDEO_MJPEG || v->format == SFX_VIDEO_PNG) return fail(SFX_E_INVALID, "video: a Motion-JPEG or PNG frame has a length of its own: sfx_video_submit_bytes");
    return video_submit(v, slot, v->frame_bytes);
}

extern "C" int sfx_video_submit_bytes(sfx_handle h, int slot, size_t nbytes) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v || slot < 0 || slot >= v->slots) return fail(SFX_E_INVALID, "invalid video handle or slot %d", slot);
    if (v->format != SFX_VIDEO_MJPEG && v->format != SFX_VIDEO_PNG) {
        if (nbytes != v->frame_bytes) return fail(SFX_E_INVALID, "video: a frame of this format has %zu bytes, not %zu", v->frame_bytes, nbytes);
        return video_submit(v, slot, nbytes);
    }
    return video_submit(v, slot, nbytes, true);
}

// The decode launches of one staged frame (jpeg_decode_kernels.hpp) on `stream`: `frame` with `intervals` restart intervals and `scan_bytes`
// bytes of scan → `rgb`. `status` is the frame's status word, cleared in front of them. Entropy decoding: a lane per interval, or, with
// `sync` (its records hold the frame's lanes: the caller has seen to that), a lane per subsequence of `subsequence` bytes with `budget`
// rounds per phase — two launches of rounds when the frame has more than one workgroup of lanes, the scan, the write pass, and the
// lane-per-interval kernel behind them, which returns at once unless the rounds did not settle. The launch sizes follow from the words
// sfx_video_submit_bytes validated. A budget of JPEG_SYNC_LANES - 1 rounds at the most: then a chain that settles in `budget` rounds of
// the whole frame settles in the two phases (phase 0 gives every lane the chain behind it in its workgroup, `budget` lanes long at the
// most; phase 1 joins the workgroups' chains). The launches run in stream order, so one frame's scratch serves every frame.
static void jpeg_launch_decode(hipStream_t stream, const uint8_t* frame, uint32_t intervals, uint32_t scan_bytes, const JpegSyncScratch* sync, uint32_t subsequence, int budget,
                               int16_t* coefficients, uint8_t* planes, const float* basis, uint32_t* status,
                               uint32_t* first_bad, uint32_t serial, uint8_t* rgb, const JpegDecodeGeometry& g, int bottom_up) {
    hipMemsetAsync(status, 0, sizeof(uint32_t), stream);
    if (sync) {
        budget = std::max(0, std::min(budget, JPEG_SYNC_LANES - 1));
        const unsigned long long lanes = jpeg_sync_lanes(scan_bytes, intervals, subsequence);
        const unsigned workgroups = (unsigned)((lanes + JPEG_SYNC_LANES - 1)/JPEG_SYNC_LANES);
        const int phases = workgroups > 1 && budget > 0 ? 2 : 1;
        for (int phase = 0; phase < phases; phase++)
            hipLaunchKernelGGL(k_jpeg_sync_rounds, dim3(workgroups), dim3(JPEG_SYNC_LANES), 0, stream, frame, *sync, g, subsequence, budget, phase);
        hipLaunchKernelGGL(k_jpeg_sync_scan, dim3(1), dim3(JPEG_SYNC_LANES), 0, stream, frame, *sync, g, subsequence, (uint32_t)workgroups, phases);
        hipLaunchKernelGGL(k_jpeg_sync_write, dim3(workgroups), dim3(JPEG_SYNC_LANES), 0, stream, frame, coefficients, status, *sync, g, subsequence);
    }
    hipLaunchKernelGGL(k_jpeg_decode_entropy, dim3((intervals + 63)/64), dim3(64), 0, stream, frame, coefficients, status, g, sync ? (const uint32_t*)sync->control : (const uint32_t*)nullptr);
    const size_t blocks = (size_t)g.mcus_x*g.mcus_y*g.blocks;
    hipLaunchKernelGGL(k_jpeg_decode_planes, dim3((unsigned)((blocks + 3)/4)), dim3(256), 0, stream, (const sfx_jpeg_frame*)frame, (const int16_t*)coefficients, planes, basis, (const uint32_t*)status,
                       (volatile uint32_t*)first_bad, serial, g);
    const long lanes = jpeg_pixel_lanes(g.width, g.height);
    hipLaunchKernelGGL(k_jpeg_decode_pixels, dim3((unsigned)((lanes + 255)/256)), dim3(256), 0, stream, (const uint8_t*)planes, rgb, (const uint32_t*)status, g, bottom_up);
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
    if (v->format == SFX_VIDEO_MJPEG) {
        // (the records hold capacity/sync_bytes lanes and an interval's each: every frame sfx_video_submit_bytes let through fits)
        const bool sync = jpeg_sync_chosen(v->scan_bytes[slot], v->intervals[slot], v->sync_bytes) && jpeg_sync_lanes(v->scan_bytes[slot], v->intervals[slot], v->sync_bytes) <= v->sync.capacity;
        (sync ? v->sync_frames : v->serial_frames)++;
        jpeg_launch_decode(v->ctx->stream, (const uint8_t*)v->staging[slot], v->intervals[slot], v->scan_bytes[slot], sync ? &v->sync : nullptr, v->sync_bytes, JPEG_SYNC_ROUNDS,
                           v->coefficients, v->planes, v->basis, v->status + slot, v->first_bad, v->serial++, (uint8_t*)front->data, v->jpeg, 1);
    } else if (v->format == SFX_VIDEO_PNG) {
        if (!v->segment_path[slot]) v->png_serial_frames++;
        png_launch_decode(v->ctx->stream, (const uint8_t*)v->staging[slot], v->staged_bytes[slot], v->segments[slot], v->segment_path[slot] != 0, v->png, v->status + slot,
                          v->first_bad, v->serial++, (uint8_t*)front->data, v->width, v->height, 1);
    } else if (v->format == SFX_VIDEO_I420) hipLaunchKernelGGL(k_video_frame<SFX_VIDEO_I420>, grid, block, 0, v->ctx->stream, (const uint8_t*)v->staging[slot], (uint8_t*)front->data, v->width, v->height);
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

// ---- Motion-JPEG sources ---------------------------------------------------------------------------------------------------------------

extern "C" int sfx_video_status(sfx_handle h, int wait, int64_t* frame, uint32_t* status) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v || !frame || !status) return fail(SFX_E_INVALID, "invalid video handle or null pointer");
    *frame = -1; *status = 0;
    if (v->format != SFX_VIDEO_MJPEG && v->format != SFX_VIDEO_PNG) return SFX_OK;      // (uncompressed frames have nothing to go wrong)
    volatile uint32_t* note = v->first_bad;
    if (!wait && note[0] == 0u) return SFX_OK;
    USE_DEVICE(v->ctx);
    HIP_TRY(hipStreamSynchronize(v->ctx->stream));
    if (note[0] != 0u) { *status = note[0]; *frame = (int64_t)note[1]; note[1] = 0u; note[0] = 0u; }
    return SFX_OK;
}

extern "C" int sfx_video_jpeg_paths(sfx_handle h, uint64_t* subsequence_frames, uint64_t* interval_frames) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v || !subsequence_frames || !interval_frames) return fail(SFX_E_INVALID, "invalid video handle or null pointer");
    std::lock_guard<std::mutex> lock(v->guard);
    *subsequence_frames = v->sync_frames; *interval_frames = v->serial_frames;
    return SFX_OK;
}

// sfx_jpeg_decode and sfx_jpeg_decode_sync. `subsequence_bytes` < 0: the lane-per-interval kernel; 0: the path a video handle would choose,
// with the production values; else the subsequence path with pieces of that size. `info`: {subsequences, rounds used, fell back} or null.
static int jpeg_decode_once(sfx_handle hc, const void* staged, size_t nbytes, int width, int height, int components, int h_sampling, int v_sampling, int subsequence_bytes,
                            int round_budget, int16_t* coefficients, uint8_t* planes, uint8_t* rgb, uint32_t* status, uint32_t* info) {
    CTX_OR_FAIL(c, hc);
    if (!staged || !status) return fail(SFX_E_INVALID, "jpeg decode: null frame or status");
    if (subsequence_bytes == 1 || subsequence_bytes > (1 << 20)) return fail(SFX_E_INVALID, "jpeg decode: subsequences of %d bytes (2 … 2^20)", subsequence_bytes);
    JpegDecodeGeometry g;
    if (const int rc = jpeg_decode_geometry(width, height, components, h_sampling, v_sampling, std::max(nbytes, (size_t)JPEG_FRAME_FIXED + 16), &g)) return rc;
    uint32_t intervals = 0, scan_bytes = 0;
    if (const char* fault = jpeg_frame_fault(staged, nbytes, g, &intervals, &scan_bytes)) return fail(SFX_E_INVALID, "jpeg decode: the staged frame of %zu bytes: %s", nbytes, fault);
    const uint32_t subsequence = subsequence_bytes > 0 ? (uint32_t)subsequence_bytes : jpeg_sync_bytes();
    const bool sync = subsequence_bytes > 0 || (subsequence_bytes == 0 && jpeg_sync_chosen(scan_bytes, intervals, subsequence));
    if (info) info[0] = info[1] = info[2] = 0u;
    USE_DEVICE(c);
    void *scratch = nullptr, *frame = nullptr, *pixels = nullptr, *records = nullptr;
    float* basis; uint32_t* device_status; int16_t* device_coefficients; uint8_t* device_planes;
    JpegSyncScratch sync_scratch{};
    const size_t rgb_bytes = (size_t)width*height*3;
    int rc = jpeg_scratch(g, 1, &scratch, &basis, &device_status, &device_coefficients, &device_planes);
    if (rc == SFX_OK && sync) rc = jpeg_sync_scratch(g, (size_t)g.capacity, subsequence, &records, &sync_scratch);
    if (rc == SFX_OK && (hipMalloc(&frame, (size_t)g.capacity) != hipSuccess || hipMalloc(&pixels, rgb_bytes) != hipSuccess)) rc = SFX_E_HIP;
    if (rc == SFX_OK) {
        bool ok = hipMemsetAsync(frame, 0, (size_t)g.capacity, c->stream) == hipSuccess && hipMemsetAsync(pixels, 0, rgb_bytes, c->stream) == hipSuccess
                  && hipMemsetAsync(device_coefficients, 0, (size_t)(device_planes - (uint8_t*)device_coefficients) + jpeg_plane_bytes(g), c->stream) == hipSuccess
                  && hipMemcpyAsync(frame, staged, nbytes, hipMemcpyHostToDevice, c->stream) == hipSuccess;
        if (ok) {
            jpeg_launch_decode(c->stream, (const uint8_t*)frame, intervals, scan_bytes, sync ? &sync_scratch : nullptr, subsequence, round_budget < 0 ? (int)JPEG_SYNC_ROUNDS : round_budget,
                               device_coefficients, device_planes, basis, device_status, nullptr, 0, (uint8_t*)pixels, g, 0);
            ok = hipGetLastError() == hipSuccess;
        }
        if (ok && coefficients) ok = hipMemcpyAsync(coefficients, device_coefficients, jpeg_decode_coefficients(g)*2, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        if (ok && planes) ok = hipMemcpyAsync(planes, device_planes, jpeg_plane_bytes(g), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        if (ok && rgb) ok = hipMemcpyAsync(rgb, pixels, rgb_bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        if (ok) ok = hipMemcpyAsync(status, device_status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        uint32_t control[3] = {0u, 0u, 0u};
        if (ok && sync) ok = hipMemcpyAsync(control, sync_scratch.control, sizeof control, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        const hipError_t synced = hipStreamSynchronize(c->stream);
        if (!ok || synced != hipSuccess) rc = fail(SFX_E_HIP, "jpeg decode: %s", hipGetErrorString(synced != hipSuccess ? synced : hipGetLastError()));
        else if (info && sync) { info[0] = control[2]; info[1] = control[1]; info[2] = control[0]; }
    } else {
        (void)hipGetLastError();
        fail(rc, "jpeg decode: the scratch of a %d x %d frame could not be allocated", width, height);
    }
    if (scratch) hipFree(scratch);
    if (records) hipFree(records);
    if (frame) hipFree(frame);
    if (pixels) hipFree(pixels);
    return rc;
}

extern "C" int sfx_jpeg_decode(sfx_handle hc, const void* staged, size_t nbytes, int width, int height, int components, int h_sampling, int v_sampling,
                               int16_t* coefficients, uint8_t* planes, uint8_t* rgb, uint32_t* status) {
    return jpeg_decode_once(hc, staged, nbytes, width, height, components, h_sampling, v_sampling, -1, 0, coefficients, planes, rgb, status, nullptr);
}

extern "C" int sfx_jpeg_decode_sync(sfx_handle hc, const void* staged, size_t nbytes, int width, int height, int components, int h_sampling, int v_sampling,
                                    int subsequence_bytes, int round_budget, int16_t* coefficients, uint8_t* planes, uint8_t* rgb, uint32_t* status, uint32_t* info) {
    if (subsequence_bytes < 0) return fail(SFX_E_INVALID, "jpeg decode: subsequences of %d bytes (0: the production rule; 2 … 2^20)", subsequence_bytes);
    return jpeg_decode_once(hc, staged, nbytes, width, height, components, h_sampling, v_sampling, subsequence_bytes, round_budget, coefficients, planes, rgb, status, info);
}

// ---- PNG sources -------------------------------------------------------------------------------------------------------------------------

extern "C" int sfx_video_png_paths(sfx_handle h, uint64_t* segment_frames, uint64_t* serial_frames) {
    Video* v = get<Video>(h, MAGIC_VIDEO);
    if (!v || !segment_frames || !serial_frames) return fail(SFX_E_INVALID, "invalid video handle or null pointer");
    *segment_frames = *serial_frames = 0;
    if (v->format != SFX_VIDEO_PNG) return SFX_OK;
    USE_DEVICE(v->ctx);
    HIP_TRY(hipStreamSynchronize(v->ctx->stream));                   // (the scan kernel of a frame says which way it went)
    std::lock_guard<std::mutex> lock(v->guard);
    volatile uint32_t* counted = v->first_bad + 4;
    *segment_frames = counted[0]; *serial_frames = v->png_serial_frames + counted[1];
    return SFX_OK;
}

extern "C" int sfx_png_decode(sfx_handle hc, const void* staged, size_t nbytes, int width, int height, int mode, uint8_t* filtered_out, uint8_t* rgb_out,
                              uint32_t* status, uint32_t* info) {
    CTX_OR_FAIL(c, hc);
    if (!staged || !status) return fail(SFX_E_INVALID, "png decode: null frame or status");
    if (mode < -1 || mode > 1) return fail(SFX_E_INVALID, "png decode: mode %d (0: serial, 1: segments, -1: as a video handle chooses)", mode);
    const size_t capacity = (std::max(nbytes, (size_t)PNG_FRAME_FIXED + 16) + 15) & ~(size_t)15;
    if (const int rc = png_geometry(width, height, capacity)) return rc;
    sfx_png_frame f;
    if (const char* fault = png_frame_fault(staged, nbytes, width, height, capacity, &f)) return fail(SFX_E_INVALID, "png decode: the staged frame of %zu bytes: %s", nbytes, fault);
    if (info) info[0] = info[1] = info[2] = 0u;
    USE_DEVICE(c);
    void *block = nullptr, *frame = nullptr, *pixels = nullptr;
    uint32_t* device_status = nullptr;
    PngScratch scratch{};
    const size_t rgb_bytes = (size_t)width*height*3, filtered_bytes = (size_t)height*(1 + 3*(size_t)width);
    int rc = png_scratch(width, height, capacity, 1, &block, &device_status, &scratch);
    if (rc == SFX_OK && (hipMalloc(&frame, capacity) != hipSuccess || hipMalloc(&pixels, rgb_bytes + 64) != hipSuccess)) rc = SFX_E_HIP;
    if (rc == SFX_OK) {
        const bool segment_path = png_segments_chosen(staged, f, scratch.capacity, mode);
        // 64 guard bytes behind the inflated stream and behind the pixels: whatever the stream says, the kernels leave them alone
        bool ok = hipMemsetAsync(frame, 0, capacity, c->stream) == hipSuccess && hipMemsetAsync(pixels, 0, rgb_bytes, c->stream) == hipSuccess
                  && hipMemsetAsync((char*)pixels + rgb_bytes, 0xa5, 64, c->stream) == hipSuccess && hipMemsetAsync(scratch.filtered + filtered_bytes, 0xa5, 64, c->stream) == hipSuccess
                  && hipMemcpyAsync(frame, staged, nbytes, hipMemcpyHostToDevice, c->stream) == hipSuccess;
        if (ok) {
            png_launch_decode(c->stream, (const uint8_t*)frame, (uint32_t)nbytes, f.segments, segment_path, scratch, device_status, nullptr, 0, (uint8_t*)pixels, width, height, 0);
            ok = hipGetLastError() == hipSuccess;
        }
        uint32_t control[2] = {0u, 0u};
        uint8_t guards[128];
        if (ok) ok = hipMemcpyAsync(guards, scratch.filtered + filtered_bytes, 64, hipMemcpyDeviceToHost, c->stream) == hipSuccess
                     && hipMemcpyAsync(guards + 64, (char*)pixels + rgb_bytes, 64, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        if (ok && filtered_out) ok = hipMemcpyAsync(filtered_out, scratch.filtered, filtered_bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        if (ok && rgb_out) ok = hipMemcpyAsync(rgb_out, pixels, rgb_bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        if (ok) ok = hipMemcpyAsync(status, device_status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) == hipSuccess
                     && hipMemcpyAsync(control, scratch.control, sizeof control, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        const hipError_t synced = hipStreamSynchronize(c->stream);
        if (!ok || synced != hipSuccess) rc = fail(SFX_E_HIP, "png decode: %s", hipGetErrorString(synced != hipSuccess ? synced : hipGetLastError()));
        else if (std::any_of(guards, guards + 128, [](uint8_t v) { return v != 0xa5; })) rc = fail(SFX_E_HIP, "png decode: the kernels wrote behind the inflated stream or behind the pixels");
        else if (info) { info[0] = f.segments; info[1] = control[0]; info[2] = segment_path ? control[1] : 0u; }
    } else {
        (void)hipGetLastError();
        fail(rc, "png decode: the scratch of a %d x %d frame could not be allocated", width, height);
    }
    if (block) hipFree(block);
    if (frame) hipFree(frame);
    if (pixels) hipFree(pixels);
    return rc;
}
