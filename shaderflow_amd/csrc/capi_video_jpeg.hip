// capi_video_jpeg.hip — the Motion-JPEG decoder of a video handle (video_decoder.hpp; the kernels: jpeg_decode_kernels.hpp):
// what a staged frame must look like, the decoder's device scratch, which entropy path a frame takes and the decode launches — and the
// entries that are Motion-JPEG's alone: sfx_video_create_mjpeg, sfx_video_jpeg_paths and the test entries sfx_jpeg_decode*.

#include "video_decoder.hpp"
#include "jpeg_decode_kernels.hpp"

#include <algorithm>
#include <cstdlib>

using namespace sf;

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

// Which entropy path a frame takes: `mode` (the test entries) or else SHADERFLOW_JPEG_SYNC = 0 / 1 force the lane-per-interval kernel /
// the subsequence path; else the subsequence path when the frame's mean restart interval holds JPEG_SYNC_RULE subsequences. (Read per
// frame: tests switch it.)
static bool jpeg_sync_chosen(uint32_t scan_bytes, uint32_t intervals, uint32_t subsequence, int mode = -1) {
    if (mode >= 0) return mode == 1;
    const char* forced = getenv("SHADERFLOW_JPEG_SYNC");
    if (forced && forced[0] == '0' && !forced[1]) return false;
    if (forced && forced[0] == '1' && !forced[1]) return true;
    return intervals > 0 && scan_bytes/intervals >= (unsigned long long)JPEG_SYNC_RULE*subsequence;
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

// Every slot holds a staged frame of its own length, at most g.capacity bytes. `mode` and `budget` are the test entries' knobs.
struct JpegDecoder : VideoDecoder {
    const JpegDecodeGeometry g;
    const uint32_t sync_bytes;                      // a subsequence's bytes on this handle
    const int mode, budget;
    std::vector<uint32_t> intervals, scan_bytes;    // restart intervals and scan bytes of the frame each slot holds
    void* scratch = nullptr;                        // [basis][status: a word per slot][coefficients][planes]
    float* basis = nullptr; uint32_t* status = nullptr; int16_t* coefficients = nullptr; uint8_t* planes = nullptr;
    void* sync_block = nullptr;                     // the subsequence path's records (jpeg_decode_kernels.hpp, 1b), for capacity/sync_bytes lanes and one per interval
    JpegSyncScratch sync{};
    uint64_t sync_frames = 0, serial_frames = 0;    // landed frames by entropy path (sfx_video_jpeg_paths)

    JpegDecoder(const JpegDecodeGeometry& geometry, uint32_t subsequence, int mode = -1, int budget = JPEG_SYNC_ROUNDS) : g(geometry), sync_bytes(subsequence), mode(mode), budget(budget) {}
    ~JpegDecoder() override { if (scratch) hipFree(scratch); if (sync_block) hipFree(sync_block); }
    const char* name() const override { return "Motion-JPEG"; }
    bool allocate(int slots) override {
        intervals.assign(slots, 0); scan_bytes.assign(slots, 0);
        return jpeg_scratch(g, slots, &scratch, &basis, &status, &coefficients, &planes) == SFX_OK && jpeg_sync_scratch(g, (size_t)g.capacity, sync_bytes, &sync_block, &sync) == SFX_OK;
    }
    const char* accept(int slot, const void* frame, size_t nbytes) override { return jpeg_frame_fault(frame, nbytes, g, &intervals[slot], &scan_bytes[slot]); }
    // (the records hold capacity/sync_bytes lanes and an interval's each: every frame `accept` let through fits)
    bool takes_sync(int slot) const {
        return jpeg_sync_chosen(scan_bytes[slot], intervals[slot], sync_bytes, mode) && jpeg_sync_lanes(scan_bytes[slot], intervals[slot], sync_bytes) <= sync.capacity;
    }
    void launch(hipStream_t stream, int slot, const uint8_t* staged, uint32_t* first_bad, uint32_t serial, uint8_t* rgb, int bottom_up) override {
        const bool chosen = takes_sync(slot);
        (chosen ? sync_frames : serial_frames)++;
        jpeg_launch_decode(stream, staged, intervals[slot], scan_bytes[slot], chosen ? &sync : nullptr, sync_bytes, budget, coefficients, planes, basis, status + slot, first_bad, serial, rgb, g, bottom_up);
    }
};

extern "C" int sfx_video_create_mjpeg(sfx_handle hc, const sfx_handle* boxes, int temporal, int width, int height, int components, int h_sampling, int v_sampling,
                                      size_t capacity, int slots, sfx_handle* out) {
    CTX_OR_FAIL(c, hc);
    JpegDecodeGeometry g;
    if (const int rc = jpeg_decode_geometry(width, height, components, h_sampling, v_sampling, capacity, &g)) return rc;
    return video_create(c, boxes, temporal, width, height, SFX_VIDEO_MJPEG, (size_t)g.capacity, slots, new JpegDecoder(g, jpeg_sync_bytes()), out);
}

extern "C" int sfx_video_jpeg_paths(sfx_handle h, uint64_t* subsequence_frames, uint64_t* interval_frames) {
    VideoDecoding v;
    if (!subsequence_frames || !interval_frames || !video_decoding(h, SFX_VIDEO_MJPEG, &v)) return fail(SFX_E_INVALID, "invalid video handle or null pointer");
    *subsequence_frames = *interval_frames = 0;
    if (!v.decoder) return SFX_OK;
    const JpegDecoder* decoder = static_cast<const JpegDecoder*>(v.decoder);
    std::lock_guard<std::mutex> lock(*v.guard);
    *subsequence_frames = decoder->sync_frames; *interval_frames = decoder->serial_frames;
    return SFX_OK;
}

// sfx_jpeg_decode and sfx_jpeg_decode_sync: the decoder a handle would have, for one slot. `subsequence_bytes` < 0: the lane-per-interval
// kernel; 0: the path a video handle would choose, with the production values; else the subsequence path with pieces of that size.
// `info`: {subsequences, rounds used, fell back} or null.
static int jpeg_decode_once(sfx_handle hc, const void* staged, size_t nbytes, int width, int height, int components, int h_sampling, int v_sampling, int subsequence_bytes,
                            int round_budget, int16_t* coefficients, uint8_t* planes, uint8_t* rgb, uint32_t* status, uint32_t* info) {
    CTX_OR_FAIL(c, hc);
    if (!staged || !status) return fail(SFX_E_INVALID, "jpeg decode: null frame or status");
    if (subsequence_bytes == 1 || subsequence_bytes > (1 << 20)) return fail(SFX_E_INVALID, "jpeg decode: subsequences of %d bytes (2 … 2^20)", subsequence_bytes);
    JpegDecodeGeometry g;
    if (const int rc = jpeg_decode_geometry(width, height, components, h_sampling, v_sampling, std::max(nbytes, (size_t)JPEG_FRAME_FIXED + 16), &g)) return rc;
    JpegDecoder decoder(g, subsequence_bytes > 0 ? (uint32_t)subsequence_bytes : jpeg_sync_bytes(), subsequence_bytes > 0 ? 1 : subsequence_bytes < 0 ? 0 : -1,
                        round_budget < 0 ? (int)JPEG_SYNC_ROUNDS : round_budget);
    if (info) info[0] = info[1] = info[2] = 0u;
    USE_DEVICE(c);
    StagedOnce once;
    const size_t rgb_bytes = (size_t)width*height*3;
    if (!decoder.allocate(1) || !once.allocate((size_t)g.capacity, rgb_bytes)) {
        (void)hipGetLastError();
        return fail(SFX_E_HIP, "jpeg decode: the scratch of a %d x %d frame could not be allocated", width, height);
    }
    if (const char* fault = decoder.accept(0, staged, nbytes)) return fail(SFX_E_INVALID, "jpeg decode: the staged frame of %zu bytes: %s", nbytes, fault);
    const bool sync = decoder.takes_sync(0);
    bool ok = once.copy_in(c->stream, staged, nbytes, (size_t)g.capacity, rgb_bytes)
              && hipMemsetAsync(decoder.coefficients, 0, (size_t)(decoder.planes - (uint8_t*)decoder.coefficients) + jpeg_plane_bytes(g), c->stream) == hipSuccess;
    if (ok) {
        decoder.launch(c->stream, 0, (const uint8_t*)once.frame, nullptr, 0, (uint8_t*)once.pixels, 0);
        ok = hipGetLastError() == hipSuccess;
    }
    if (ok && coefficients) ok = hipMemcpyAsync(coefficients, decoder.coefficients, jpeg_decode_coefficients(g)*2, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (ok && planes) ok = hipMemcpyAsync(planes, decoder.planes, jpeg_plane_bytes(g), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (ok && rgb) ok = hipMemcpyAsync(rgb, once.pixels, rgb_bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (ok) ok = hipMemcpyAsync(status, decoder.status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    uint32_t control[3] = {0u, 0u, 0u};
    if (ok && sync) ok = hipMemcpyAsync(control, decoder.sync.control, sizeof control, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    const int rc = once.finish(c->stream, ok, "jpeg decode");
    if (rc == SFX_OK && info && sync) { info[0] = control[2]; info[1] = control[1]; info[2] = control[0]; }
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
