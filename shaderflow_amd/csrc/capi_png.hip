// capi_png.hip — the C-ABI's PNG half (include/shaderflow_hip.h: sfx_png_*): an encoder object with its constants on the device, and
// the three launches of png_kernels.hpp on the context's render stream. The stream is defined in png_kernels.hpp; DESIGN.md §7d has
// the mapping and the capacity argument.

#include "host_state.hpp"
#include "png_kernels.hpp"

#include <algorithm>

using namespace sf;

enum : uint32_t { MAGIC_PNG = 0x53465850 };

struct PngEncoder : Object {
    Context* ctx;
    PngGeometry geometry;
    PngTables tables;
    void* constants = nullptr;                                      // the CRC's shift multipliers
    // per launch, for `capacity` frames (grown on demand): the filtered streams, the rows' Adler sums, the stripes' chunk data, lengths and CRCs
    int capacity = 0, last_frame = -1;
    uint8_t* filtered = nullptr; uint32_t* sums = nullptr; uint8_t* segments = nullptr; uint32_t* lengths = nullptr; uint32_t* crcs = nullptr;
    size_t filtered_bytes() const { return (size_t)geometry.height*geometry.row_bytes; }
};

static uint32_t crc_register(uint32_t c, const uint8_t* data, size_t count) {
    for (size_t k = 0; k < count; k++) {
        c ^= data[k];
        for (int bit = 0; bit < 8; bit++) c = (c >> 1) ^ ((c & 1u) ? PNG_CRC_POLY : 0u);
    }
    return c;
}

// bytes a stripe of n filtered bytes takes at the most, framing included (png_kernels.hpp: the fixed-block fallback)
static size_t stripe_bound(size_t n) { return (9*n + 7)/8 + 16; }

static bool png_sizes(int width, int height, PngGeometry& g) {
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return false;
    g.width = width; g.height = height; g.row_bytes = 1 + 3*width; g.bottom_up = 0;
    g.stripes = (height + PNG_STRIPE_ROWS - 1)/PNG_STRIPE_ROWS;
    size_t total = 57 + 6;
    for (int y = 0; y < height; y += PNG_STRIPE_ROWS) total += stripe_bound((size_t)std::min(PNG_STRIPE_ROWS, height - y)*g.row_bytes) + 12;
    total = (total + 15) & ~(size_t)15;
    if (total > 0x7fffffffu) return false;
    g.payload_capacity = (int)total;
    // (zlib header and Adler-32 ride in the first and the last stripe's segment; whole 16-byte stores)
    g.segment_capacity = (int)((stripe_bound((size_t)PNG_STRIPE_ROWS*g.row_bytes) + 6 + 15) & ~(size_t)15);
    return true;
}

extern "C" int sfx_png_capacity(int width, int height, size_t* bytes) {
    PngGeometry g;
    if (!bytes || !png_sizes(width, height, g)) return fail(SFX_E_INVALID, "png capacity of %dx%d (extents 1…65535, a frame below 2 GiB)", width, height);
    *bytes = (size_t)g.payload_capacity;
    return SFX_OK;
}

extern "C" int sfx_png_create(sfx_handle h, int width, int height, sfx_handle* out) {
    CTX_OR_FAIL(c, h);
    PngGeometry g;
    if (!out || !png_sizes(width, height, g)) return fail(SFX_E_INVALID, "png encoder of %dx%d (extents 1…65535, a frame below 2 GiB)", width, height);
    USE_DEVICE(c);
    PngEncoder* e = new PngEncoder();
    e->magic = MAGIC_PNG; e->ctx = c; e->geometry = g;

    const uint8_t ihdr[17] = {'I', 'H', 'D', 'R', (uint8_t)(width >> 24), (uint8_t)(width >> 16), (uint8_t)(width >> 8), (uint8_t)width,
                              (uint8_t)(height >> 24), (uint8_t)(height >> 16), (uint8_t)(height >> 8), (uint8_t)height, 8, 2, 0, 0, 0};
    const uint8_t start[12] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n', 0, 0, 0, 13};
    const uint32_t crc = ~crc_register(0xffffffffu, ihdr, sizeof(ihdr));
    memset(e->tables.head, 0, sizeof(e->tables.head));
    memcpy(e->tables.head, start, 12);
    memcpy(e->tables.head + 12, ihdr, 17);
    for (int k = 0; k < 4; k++) e->tables.head[29 + k] = (uint8_t)(crc >> (24 - 8*k));
    e->tables.idat_state = crc_register(0xffffffffu, (const uint8_t*)"IDAT", 4);

    uint32_t shift[PNG_SHIFTS];
    uint32_t power = 0x80000000u;                                   // x^0
    for (int k = 0; k < PNG_SHIFTS; k++) {
        shift[k] = power;
        for (int bit = 0; bit < 128; bit++) power = (power >> 1) ^ ((power & 1u) ? PNG_CRC_POLY : 0u);
    }
    if (hipMalloc(&e->constants, sizeof(shift)) != hipSuccess || hipMemcpy(e->constants, shift, sizeof(shift), hipMemcpyHostToDevice) != hipSuccess) {
        const hipError_t err = hipGetLastError();
        if (e->constants) hipFree(e->constants);
        delete e;
        return fail(SFX_E_HIP, "png encoder constants: %s", hipGetErrorString(err));
    }
    e->tables.shift = (const uint32_t*)e->constants;
    *out = handle_of(e);
    return SFX_OK;
}

static void png_release_scratch(PngEncoder* e) {
    for (void* p : {(void*)e->filtered, (void*)e->sums, (void*)e->segments, (void*)e->lengths, (void*)e->crcs}) if (p) hipFree(p);
    e->filtered = nullptr; e->sums = nullptr; e->segments = nullptr; e->lengths = nullptr; e->crcs = nullptr; e->capacity = 0; e->last_frame = -1;
}

extern "C" int sfx_png_destroy(sfx_handle h) {
    PngEncoder* e = get<PngEncoder>(h, MAGIC_PNG);
    if (!e) return fail(SFX_E_INVALID, "invalid png encoder handle");
    hipSetDevice(e->ctx->device);
    hipStreamSynchronize(e->ctx->stream);
    png_release_scratch(e);
    hipFree(e->constants);
    e->magic = 0;
    delete e;
    return SFX_OK;
}

// `frames` RGB8 frames (consecutive, width*height*3 bytes each) → sink frames (consecutive, 64 + sfx_png_capacity bytes each), one
// launch per stage and per group of frames that fits the encoder's scratch (512 MiB of filtered streams and chunk data at the most)
extern "C" int sfx_png_encode(sfx_handle h, const void* rgb, void* sink, int frames, int bottom_up) {
    PngEncoder* e = get<PngEncoder>(h, MAGIC_PNG);
    if (!e || !rgb || !sink || frames < 1) return fail(SFX_E_INVALID, "png encode: invalid encoder handle, pointer or frame count");
    if ((uintptr_t)sink & 3) return fail(SFX_E_INVALID, "png encode: the sink frames must be 4-byte aligned");
    Context* c = e->ctx;
    USE_DEVICE(c);
    PngGeometry g = e->geometry;
    g.bottom_up = bottom_up ? 1 : 0;
    const size_t segment_bytes = (size_t)g.stripes*g.segment_capacity;
    const size_t per_frame = e->filtered_bytes() + segment_bytes;
    const int group = (int)std::max<size_t>(1, std::min<size_t>({(size_t)frames, (size_t)1024, ((size_t)512 << 20)/per_frame}));
    if (group > e->capacity) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        png_release_scratch(e);
        HIP_TRY(hipMalloc((void**)&e->filtered, e->filtered_bytes()*group));
        HIP_TRY(hipMalloc((void**)&e->sums, sizeof(uint32_t)*2*g.height*group));
        HIP_TRY(hipMalloc((void**)&e->segments, segment_bytes*group));
        HIP_TRY(hipMalloc((void**)&e->lengths, sizeof(uint32_t)*g.stripes*group));
        HIP_TRY(hipMalloc((void**)&e->crcs, sizeof(uint32_t)*g.stripes*group));
        e->capacity = group;
    }
    const size_t sink_stride = PNG_SINK_HEADER + (size_t)g.payload_capacity, rgb_stride = (size_t)g.width*g.height*3;
    for (int first = 0; first < frames; first += group) {
        const int n = std::min(group, frames - first);
        const uint8_t* source = (const uint8_t*)rgb + first*rgb_stride;
        uint8_t* target = (uint8_t*)sink + first*sink_stride;
        hipLaunchKernelGGL(k_png_filter, dim3(g.height, 1, n), dim3(256), 0, c->stream, source, e->filtered, e->sums, g);
        hipLaunchKernelGGL(k_png_deflate, dim3(g.stripes, 1, n), dim3(64), 0, c->stream, (const uint8_t*)e->filtered, (const uint32_t*)e->sums, e->segments, e->lengths, e->crcs, e->tables, g);
        hipLaunchKernelGGL(k_png_pack, dim3(g.stripes, 1, n), dim3(256), 0, c->stream, (const uint8_t*)e->segments, (const uint32_t*)e->lengths, (const uint32_t*)e->crcs, target, sink_stride, e->tables, g);
        e->last_frame = n - 1;
    }
    return launch_status();
}

// the last encoded frame's filtered stream: height rows of 1 + 3*width bytes (the filter type, the filtered bytes). Synchronous.
extern "C" int sfx_png_filtered(sfx_handle h, uint8_t* out) {
    PngEncoder* e = get<PngEncoder>(h, MAGIC_PNG);
    if (!e || !out) return fail(SFX_E_INVALID, "invalid png encoder handle or null pointer");
    if (e->last_frame < 0) return fail(SFX_E_INVALID, "png filtered: nothing has been encoded yet");
    USE_DEVICE(e->ctx);
    HIP_TRY(hipMemcpyAsync(out, e->filtered + (size_t)e->last_frame*e->filtered_bytes(), e->filtered_bytes(), hipMemcpyDeviceToHost, e->ctx->stream));
    HIP_TRY(hipStreamSynchronize(e->ctx->stream));
    return SFX_OK;
}

// the tables step of k_png_deflate on a histogram of the caller's: 286 literal/length counts, then 30 distance counts. Synchronous.
extern "C" int sfx_png_code_lengths(sfx_handle h, const uint32_t* histogram, uint8_t* lengths, int* fixed) {
    CTX_OR_FAIL(c, h);
    if (!histogram || !lengths || !fixed) return fail(SFX_E_INVALID, "png code lengths: null pointer");
    unsigned long long total = 0;
    for (int k = 0; k < PNG_SYMBOLS; k++) total += histogram[k];
    if (total > 0x0fffffffull) return fail(SFX_E_INVALID, "png code lengths: the counts add up to %llu (2^28 - 1 at the most)", total);
    USE_DEVICE(c);
    struct Device { uint32_t histogram[PNG_SYMBOLS]; int fixed; uint8_t lengths[PNG_SYMBOLS]; };
    Device* device = nullptr;
    HIP_TRY(hipMalloc((void**)&device, sizeof(Device)));
    int status = SFX_OK;
    Device host;
    if (hipMemcpyAsync(device->histogram, histogram, sizeof(host.histogram), hipMemcpyHostToDevice, c->stream) != hipSuccess) status = fail(SFX_E_HIP, "png code lengths: upload");
    if (status == SFX_OK) {
        hipLaunchKernelGGL(k_png_tables, dim3(1), dim3(64), 0, c->stream, (const uint32_t*)device->histogram, device->lengths, &device->fixed);
        status = launch_status();
    }
    if (status == SFX_OK && (hipMemcpyAsync(&host, device, sizeof(Device), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess))
        status = fail(SFX_E_HIP, "png code lengths: %s", hipGetErrorString(hipGetLastError()));
    hipStreamSynchronize(c->stream);
    hipFree(device);
    if (status != SFX_OK) return status;
    memcpy(lengths, host.lengths, PNG_SYMBOLS);
    *fixed = host.fixed;
    return SFX_OK;
}
