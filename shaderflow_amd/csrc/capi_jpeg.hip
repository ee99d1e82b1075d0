// capi_jpeg.hip — the C-ABI's Motion-JPEG half (include/shaderflow_hip.h: sfx_jpeg_*): an encoder object with its tables and constant
// header on the device, and the three launches of jpeg_kernels.hpp on the context's render stream. The stream is defined in
// jpeg_kernels.hpp; DESIGN.md §7b has the mapping.

#include "host_state.hpp"
#include "jpeg_kernels.hpp"

#include <algorithm>
#include <cmath>

using namespace sf;

enum : uint32_t { MAGIC_JPEG = 0x5346584a };

struct JpegEncoder : Object {
    Context* ctx;
    int width, height, quality;
    JpegGeometry geometry;
    JpegTables tables;
    void* constants = nullptr;                                      // dct, reciprocals, Huffman entries, header: one allocation
    std::vector<uint8_t> header;
    // per launch: coefficients, the intervals' segments and their lengths of `capacity` frames (grown on demand)
    int capacity = 0, last_frame = -1;                              // last_frame: where in `coefficients` the last encoded frame's terms are
    int16_t* coefficients = nullptr; uint8_t* segments = nullptr; uint32_t* lengths = nullptr;
    size_t coefficient_count() const { return (size_t)geometry.mcus_x*geometry.mcus_y*384; }
};

static void put16(std::vector<uint8_t>& out, int v) { out.push_back((uint8_t)(v >> 8)); out.push_back((uint8_t)v); }

// (length << 16) | code of every symbol of a table, at `entries[symbol]` (Annex C)
static void huffman_entries(const uint8_t* bits, const uint8_t* values, uint32_t* entries) {
    uint32_t code = 0; int k = 0;
    for (int length = 1; length <= 16; length++) {
        for (int n = 0; n < bits[length - 1]; n++) entries[values[k++]] = ((uint32_t)length << 16) | code++;
        code <<= 1;
    }
}

extern "C" int sfx_jpeg_create(sfx_handle h, int width, int height, int quality, sfx_handle* out) {
    CTX_OR_FAIL(c, h);
    if (!out || width < 1 || height < 1 || width > 65535 || height > 65535 || quality < 1 || quality > 100)
        return fail(SFX_E_INVALID, "jpeg encoder of %dx%d at quality %d (extents 1…65535, quality 1…100)", width, height, quality);
    USE_DEVICE(c);
    JpegEncoder* e = new JpegEncoder();
    e->magic = MAGIC_JPEG; e->ctx = c; e->width = width; e->height = height; e->quality = quality;
    JpegGeometry& g = e->geometry;
    g.width = width; g.height = height; g.mcus_x = (width + 15)/16; g.mcus_y = (height + 15)/16; g.bottom_up = 0;
    if ((long long)g.mcus_x*16*g.mcus_y*16*3 > 0x7fffffffLL) { delete e; return fail(SFX_E_TOO_LARGE, "jpeg encoder: %dx%d", width, height); }
    g.segment_capacity = 16*g.mcus_x*16*3;
    g.payload_capacity = g.mcus_x*16*g.mcus_y*16*3;

    uint8_t quant[2][64];
    const int scale = quality < 50 ? 5000/quality : 200 - 2*quality;
    for (int k = 0; k < 64; k++) {
        quant[0][k] = (uint8_t)std::min(255, std::max(1, (LUMINANCE[k]*scale + 50)/100));
        quant[1][k] = (uint8_t)std::min(255, std::max(1, (CHROMINANCE[k]*scale + 50)/100));
    }

    std::vector<uint8_t>& hd = e->header;
    hd = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int t = 0; t < 2; t++) {
        hd.insert(hd.end(), {0xff, 0xdb, 0, 67, (uint8_t)t});
        for (int n = 0; n < 64; n++) hd.push_back(quant[t][JPEG_ZIGZAG.natural_of[n]]);
    }
    hd.insert(hd.end(), {0xff, 0xc0, 0, 17, 8});
    put16(hd, height); put16(hd, width);
    hd.insert(hd.end(), {3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    struct { uint8_t selector; const uint8_t* bits; const uint8_t* values; int count; } huffman[4] = {
        {0x00, DC_LUMINANCE_BITS, DC_LUMINANCE_VALUES, 12}, {0x10, AC_LUMINANCE_BITS, AC_LUMINANCE_VALUES, 162},
        {0x01, DC_CHROMINANCE_BITS, DC_CHROMINANCE_VALUES, 12}, {0x11, AC_CHROMINANCE_BITS, AC_CHROMINANCE_VALUES, 162}};
    for (auto& t : huffman) {
        hd.insert(hd.end(), {0xff, 0xc4});
        put16(hd, 19 + t.count);
        hd.push_back(t.selector);
        hd.insert(hd.end(), t.bits, t.bits + 16);
        hd.insert(hd.end(), t.values, t.values + t.count);
    }
    hd.insert(hd.end(), {0xff, 0xdd, 0, 4});
    put16(hd, g.mcus_x);
    hd.insert(hd.end(), {0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});

    // device constants: [dct 64 f32][reciprocal 128 f32][huffman 544 u32][header]
    struct { float dct[64]; float reciprocal[128]; uint32_t huffman[2*272]; uint8_t header[JPEG_MAX_HEADER]; } host{};
    static_assert(sizeof(host) == 64*4 + 128*4 + 544*4 + JPEG_MAX_HEADER, "packed");
    jpeg_dct_basis(host.dct);
    for (int t = 0; t < 2; t++) for (int k = 0; k < 64; k++) host.reciprocal[t*64 + k] = 1.0f/(float)quant[t][k];
    huffman_entries(DC_LUMINANCE_BITS, DC_LUMINANCE_VALUES, host.huffman);
    huffman_entries(AC_LUMINANCE_BITS, AC_LUMINANCE_VALUES, host.huffman + 16);
    huffman_entries(DC_CHROMINANCE_BITS, DC_CHROMINANCE_VALUES, host.huffman + 272);
    huffman_entries(AC_CHROMINANCE_BITS, AC_CHROMINANCE_VALUES, host.huffman + 272 + 16);
    if (hd.size() > JPEG_MAX_HEADER) { delete e; return fail(SFX_E_INVALID, "jpeg header of %zu bytes", hd.size()); }
    memcpy(host.header, hd.data(), hd.size());
    if (hipMalloc(&e->constants, sizeof(host)) != hipSuccess || hipMemcpy(e->constants, &host, sizeof(host), hipMemcpyHostToDevice) != hipSuccess) {
        const hipError_t err = hipGetLastError();
        if (e->constants) hipFree(e->constants);
        delete e;
        return fail(SFX_E_HIP, "jpeg encoder tables: %s", hipGetErrorString(err));
    }
    const char* base = (const char*)e->constants;
    e->tables.dct = (const float*)base;
    e->tables.reciprocal = (const float*)(base + 64*4);
    e->tables.huffman = (const uint32_t*)(base + 192*4);
    e->tables.header = (const uint8_t*)(base + 192*4 + 544*4);
    e->tables.header_bytes = (int)hd.size();
    *out = handle_of(e);
    return SFX_OK;
}

static void jpeg_release_scratch(JpegEncoder* e) {
    if (e->coefficients) hipFree(e->coefficients);
    if (e->segments) hipFree(e->segments);
    if (e->lengths) hipFree(e->lengths);
    e->coefficients = nullptr; e->segments = nullptr; e->lengths = nullptr; e->capacity = 0; e->last_frame = -1;
}

extern "C" int sfx_jpeg_destroy(sfx_handle h) {
    JpegEncoder* e = get<JpegEncoder>(h, MAGIC_JPEG);
    if (!e) return fail(SFX_E_INVALID, "invalid jpeg encoder handle");
    hipSetDevice(e->ctx->device);
    hipStreamSynchronize(e->ctx->stream);
    jpeg_release_scratch(e);
    hipFree(e->constants);
    e->magic = 0;
    delete e;
    return SFX_OK;
}

// `frames` RGB8 frames (consecutive, width*height*3 bytes each) → sink frames (consecutive, 64 + Wp*Hp*3 bytes each), one launch per
// stage and per group of frames that fits the encoder's scratch (512 MiB of coefficients and segments at the most)
extern "C" int sfx_jpeg_encode(sfx_handle h, const void* rgb, void* sink, int frames, int bottom_up) {
    JpegEncoder* e = get<JpegEncoder>(h, MAGIC_JPEG);
    if (!e || !rgb || !sink || frames < 1) return fail(SFX_E_INVALID, "jpeg encode: invalid encoder handle, pointer or frame count");
    if ((uintptr_t)sink & 3) return fail(SFX_E_INVALID, "jpeg encode: the sink frames must be 4-byte aligned");
    Context* c = e->ctx;
    USE_DEVICE(c);
    JpegGeometry g = e->geometry;
    g.bottom_up = bottom_up ? 1 : 0;
    const size_t per_frame = e->coefficient_count()*2 + (size_t)g.payload_capacity;
    const int group = (int)std::max<size_t>(1, std::min<size_t>({(size_t)frames, (size_t)1024, ((size_t)512 << 20)/per_frame}));
    if (group > e->capacity) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        jpeg_release_scratch(e);
        HIP_TRY(hipMalloc((void**)&e->coefficients, e->coefficient_count()*2*group));
        HIP_TRY(hipMalloc((void**)&e->segments, (size_t)g.payload_capacity*group));
        HIP_TRY(hipMalloc((void**)&e->lengths, sizeof(uint32_t)*g.mcus_y*group));
        e->capacity = group;
    }
    const size_t sink_stride = JPEG_SINK_HEADER + (size_t)g.payload_capacity, rgb_stride = (size_t)g.width*g.height*3;
    for (int first = 0; first < frames; first += group) {
        const int n = std::min(group, frames - first);
        const uint8_t* source = (const uint8_t*)rgb + first*rgb_stride;
        uint8_t* target = (uint8_t*)sink + first*sink_stride;
        hipLaunchKernelGGL(k_jpeg_coefficients, dim3(g.mcus_x, g.mcus_y, n), dim3(384), 0, c->stream, source, e->coefficients, e->tables, g);
        hipLaunchKernelGGL(k_jpeg_entropy, dim3(g.mcus_y, 1, n), dim3(64), 0, c->stream, (const int16_t*)e->coefficients, e->segments, e->lengths, e->tables, g);
        hipLaunchKernelGGL(k_jpeg_pack, dim3(g.mcus_y, 1, n), dim3(256), 0, c->stream, (const uint8_t*)e->segments, (const uint32_t*)e->lengths, target, sink_stride, e->tables, g);
        e->last_frame = n - 1;
    }
    return launch_status();
}

extern "C" int sfx_jpeg_header(sfx_handle h, void* buffer, size_t* count) {
    JpegEncoder* e = get<JpegEncoder>(h, MAGIC_JPEG);
    if (!e || !count) return fail(SFX_E_INVALID, "invalid jpeg encoder handle or null count");
    if (buffer) {
        if (*count < e->header.size()) return fail(SFX_E_INVALID, "jpeg header: %zu bytes, the buffer holds %zu", e->header.size(), *count);
        memcpy(buffer, e->header.data(), e->header.size());
    }
    *count = e->header.size();
    return SFX_OK;
}

// the last encoded frame's quantised terms: mcu rows x mcus per row x (Y0 Y1 Y2 Y3 Cb Cr) x 64 in zigzag order. Synchronous.
extern "C" int sfx_jpeg_coefficients(sfx_handle h, int16_t* out) {
    JpegEncoder* e = get<JpegEncoder>(h, MAGIC_JPEG);
    if (!e || !out) return fail(SFX_E_INVALID, "invalid jpeg encoder handle or null pointer");
    if (e->last_frame < 0) return fail(SFX_E_INVALID, "jpeg coefficients: nothing has been encoded yet");
    USE_DEVICE(e->ctx);
    HIP_TRY(hipMemcpyAsync(out, e->coefficients + (size_t)e->last_frame*e->coefficient_count(), e->coefficient_count()*2, hipMemcpyDeviceToHost, e->ctx->stream));
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    return SFX_OK;
}
