// capi_jpeg.hip — the C-ABI's Motion-JPEG half (include/shaderflow_hip.h: sfx_jpeg_*): an encoder object with its tables and constant
// header on the device, and the three launches of jpeg_kernels.hpp on the context's render stream. The stream is defined in
// jpeg_kernels.hpp; DESIGN.md §7b has the mapping.

#include "host_state.hpp"
#include "jpeg_kernels.hpp"

#include <algorithm>
#include <cmath>

using namespace sf;

enum : uint32_t { MAGIC_JPEG = 0x5346584a };

// the standard's Annex K tables: quantisation in natural order, Huffman as BITS / HUFFVAL
static const uint8_t LUMINANCE[64] = {
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99,
};
static const uint8_t CHROMINANCE[64] = {
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
};
static const uint8_t DC_LUMINANCE_BITS[16] = {
    0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0,
};
static const uint8_t DC_LUMINANCE_VALUES[12] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};
static const uint8_t DC_CHROMINANCE_BITS[16] = {
    0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0,
};
static const uint8_t DC_CHROMINANCE_VALUES[12] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11,
};
static const uint8_t AC_LUMINANCE_BITS[16] = {
    0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125,
};
static const uint8_t AC_LUMINANCE_VALUES[162] = {
    1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177,
    193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55,
    56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106,
    115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
    164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
    212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250,
};
static const uint8_t AC_CHROMINANCE_BITS[16] = {
    0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119,
};
static const uint8_t AC_CHROMINANCE_VALUES[162] = {
    0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193,
    9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54,
    55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105,
    106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
    162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
    210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250,
};

struct JpegEncoder : Object {
    Context* ctx;
    int width, height, quality;
    JpegGeometry geometry;
    JpegTables tables;
    void* constants = nullptr;                                      // dct, reciprocals, zigzag, Huffman entries, header: one allocation
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

    uint8_t quant[2][64], zigzag_of[64], natural_of[64];
    const int scale = quality < 50 ? 5000/quality : 200 - 2*quality;
    for (int k = 0; k < 64; k++) {
        quant[0][k] = (uint8_t)std::min(255, std::max(1, (LUMINANCE[k]*scale + 50)/100));
        quant[1][k] = (uint8_t)std::min(255, std::max(1, (CHROMINANCE[k]*scale + 50)/100));
    }
    for (int sum = 0, n = 0; sum < 15; sum++)                       // the zigzag walk: anti-diagonals, alternating direction
        for (int k = 0; k <= sum; k++) {
            const int row = (sum & 1) ? k : sum - k, col = sum - row;
            if (row < 8 && col < 8) { natural_of[n] = (uint8_t)(row*8 + col); zigzag_of[row*8 + col] = (uint8_t)n; n++; }
        }

    std::vector<uint8_t>& hd = e->header;
    hd = {0xff, 0xd8, 0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int t = 0; t < 2; t++) {
        hd.insert(hd.end(), {0xff, 0xdb, 0, 67, (uint8_t)t});
        for (int n = 0; n < 64; n++) hd.push_back(quant[t][natural_of[n]]);
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

    // device constants: [dct 64 f32][reciprocal 128 f32][huffman 544 u32][zigzag 64 u8][header]
    struct { float dct[64]; float reciprocal[128]; uint32_t huffman[2*272]; uint8_t zigzag_of[64]; uint8_t header[JPEG_MAX_HEADER]; } host{};
    static_assert(sizeof(host) == 64*4 + 128*4 + 544*4 + 64 + JPEG_MAX_HEADER, "packed");
    for (int u = 0; u < 8; u++)
        for (int x = 0; x < 8; x++) host.dct[u*8 + x] = (float)((u == 0 ? std::sqrt(0.125) : 0.5)*std::cos((2*x + 1)*u*M_PI/16.0));
    for (int t = 0; t < 2; t++) for (int k = 0; k < 64; k++) host.reciprocal[t*64 + k] = 1.0f/(float)quant[t][k];
    huffman_entries(DC_LUMINANCE_BITS, DC_LUMINANCE_VALUES, host.huffman);
    huffman_entries(AC_LUMINANCE_BITS, AC_LUMINANCE_VALUES, host.huffman + 16);
    huffman_entries(DC_CHROMINANCE_BITS, DC_CHROMINANCE_VALUES, host.huffman + 272);
    huffman_entries(AC_CHROMINANCE_BITS, AC_CHROMINANCE_VALUES, host.huffman + 272 + 16);
    memcpy(host.zigzag_of, zigzag_of, 64);
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
    e->tables.zigzag_of = (const uint8_t*)(base + 192*4 + 544*4);
    e->tables.header = e->tables.zigzag_of + 64;
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
