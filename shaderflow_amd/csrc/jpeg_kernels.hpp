// jpeg_kernels.hpp — baseline JPEG of RGB8 frames on the device (capi_jpeg.hip launches these).
//
// The stream is DEFINED here, like the yuv420p bytes (capi_readout.hip), and restated in float64 by tests/jpeg_ref.py:
//   * the frame is read top row first (`bottom_up`: the frame's rows are stored bottom-up and are read in reverse) and completed to whole
//     16 x 16 MCUs by repeating the last column and the last row of RGB pixels;
//   * colour, full range, 8-bit integer coefficients, arithmetic shifts, each clipped to 0…255:
//       Y  =  (77 R + 150 G +  29 B + 128) >> 8
//       Cb = ((-43 R -  85 G + 128 B + 128) >> 8) + 128
//       Cr = ((128 R - 107 G -  21 B + 128) >> 8) + 128
//     luma per pixel, chroma from the rounded mean of the 2 x 2 block's R, G and B ((sum + 2) >> 2), as k_rgb_to_yuv420 does;
//   * level shift by 128, 8 x 8 forward DCT-II in f32 with the standard's orthonormal scaling (rows, then columns);
//   * quantise: round-half-away(c/q) (here c times the f32 reciprocal of q), AC terms clamped to ±1023; zigzag order;
//   * 4:2:0, MCU = Y0 Y1 Y2 Y3 Cb Cr, the standard's Annex K Huffman tables, one restart interval per MCU row.
//
// Three kernels, grid.z = frames: k_jpeg_coefficients (one block per MCU), k_jpeg_entropy (one wave per restart interval, a lane per
// zigzag index), k_jpeg_pack (one block per interval: its segment behind the constant header, RSTn between, EOI and the sink frame's
// header behind the last).
#pragma once

#include "jpeg_common.hpp"

namespace sf {

constexpr uint32_t JPEG_SINK_MAGIC = 0x504a4653u;                   // "SFJP": first word of a sink frame's 64-byte header
constexpr int JPEG_SINK_HEADER = 64;                                // [magic, payload bytes, status, 0…] then the payload
constexpr uint32_t JPEG_OVERFLOW = 0xffffffffu;                     // a segment's length when its interval did not fit its capacity
constexpr int JPEG_MAX_HEADER = 1024;

// what the three kernels read of an encoder (device pointers; built once by sfx_jpeg_create)
struct JpegTables {
    const float* dct;               // [8][8]: dct[u][x] = C(u)/2 cos((2x + 1) u pi / 16)
    const float* reciprocal;        // [2][64] natural order: 1/q of luminance, chrominance
    const uint32_t* huffman;        // [2][16 DC + 256 AC]: (length << 16) | code; luminance, chrominance
    const uint8_t* header;          // SOI … SOS
    int header_bytes;
};

struct JpegGeometry {
    int width, height;              // the picture
    int mcus_x, mcus_y;             // MCUs per row (= the restart interval), MCU rows
    int segment_capacity;           // bytes an interval's entropy-coded segment may take: 16 * Wp * 3
    int payload_capacity;           // Wp * Hp * 3
    int bottom_up;
};

// ---- 1. colour, chroma mean, DCT, quantisation ------------------------------------------------------------------------------------
// One block of 384 threads per MCU: 256 of them load a pixel each, 64 make a chroma sample each, then every thread owns one term of
// the six 8 x 8 blocks in both passes (8 multiply-adds from LDS per pass) and stores one int16.
__global__ void __launch_bounds__(384) k_jpeg_coefficients(const uint8_t* __restrict__ rgb, int16_t* __restrict__ coefficients, JpegTables tables, JpegGeometry g) {
    __shared__ float dct[64];
    __shared__ int pixels[16][16][3];
    __shared__ float block[6][8][8];
    __shared__ float rows[6][8][8];
    const int t = threadIdx.x;
    const uint8_t* frame = rgb + (size_t)blockIdx.z*g.width*g.height*3;
    if (t < 64) dct[t] = tables.dct[t];
    if (t < 256) {
        const int px = t & 15, py = t >> 4;
        const int x = min((int)blockIdx.x*16 + px, g.width - 1), y = min((int)blockIdx.y*16 + py, g.height - 1);
        const uint8_t* p = frame + ((size_t)(g.bottom_up ? g.height - 1 - y : y)*g.width + x)*3;
        const int r = p[0], gr = p[1], b = p[2];
        pixels[py][px][0] = r; pixels[py][px][1] = gr; pixels[py][px][2] = b;
        const int luma = min(255, max(0, (77*r + 150*gr + 29*b + 128) >> 8));
        block[(py >> 3)*2 + (px >> 3)][py & 7][px & 7] = (float)(luma - 128);
    }
    __syncthreads();
    if (t < 64) {
        const int cx = t & 7, cy = t >> 3;
        int sum[3];
#pragma unroll
        for (int k = 0; k < 3; k++) sum[k] = (pixels[2*cy][2*cx][k] + pixels[2*cy][2*cx + 1][k] + pixels[2*cy + 1][2*cx][k] + pixels[2*cy + 1][2*cx + 1][k] + 2) >> 2;
        const int cb = min(255, max(0, ((-43*sum[0] - 85*sum[1] + 128*sum[2] + 128) >> 8) + 128));
        const int cr = min(255, max(0, ((128*sum[0] - 107*sum[1] - 21*sum[2] + 128) >> 8) + 128));
        block[4][cy][cx] = (float)(cb - 128);
        block[5][cy][cx] = (float)(cr - 128);
    }
    __syncthreads();
    const int b = t >> 6, v = (t >> 3) & 7, u = t & 7;
    float acc = 0.0f;
#pragma unroll
    for (int x = 0; x < 8; x++) acc = fmaf(block[b][v][x], dct[u*8 + x], acc);          // row v of the block, frequency u along it
    rows[b][v][u] = acc;
    __syncthreads();
    acc = 0.0f;
#pragma unroll
    for (int y = 0; y < 8; y++) acc = fmaf(rows[b][y][u], dct[v*8 + y], acc);           // column u, frequency v down it
    const int natural = v*8 + u;
    const float scaled = acc*tables.reciprocal[(b >= 4 ? 64 : 0) + natural];
    int q = (int)truncf(scaled + copysignf(0.5f, scaled));                               // round half away from zero
    if (natural) q = min(1023, max(-1023, q));
    const size_t mcu = ((size_t)blockIdx.z*g.mcus_y + blockIdx.y)*g.mcus_x + blockIdx.x;
    coefficients[mcu*384 + b*64 + JPEG_ZIGZAG.zigzag_of[natural]] = (int16_t)q;
}

// ---- 2. Huffman coding of one restart interval per wave ------------------------------------------------------------------------------
// Lane = zigzag index of the current block. A lane's contribution is at most 3 ZRL codes (11 bits each), a code of up to 16 bits and 10
// extra bits: 59 bits in a 64-bit word. A block's bits are OR-ed into an LDS bit buffer (big-endian words) behind the bits the last
// block left over (< 8), its whole bytes are stuffed (FF → FF 00) into an LDS byte stage, and the stage leaves for the interval's
// segment 1 KiB at a time in 16-byte stores.
constexpr int JPEG_BIT_WORDS = 64;                                  // 2048 bits ≥ 7 + 20 + 63*26
constexpr int JPEG_STAGE_FLUSH = 1024, JPEG_STAGE_BYTES = JPEG_STAGE_FLUSH + 512;   // a block adds at most 2*210 bytes

__device__ __forceinline__ int jpeg_wave_scan(int value, int lane) {           // inclusive prefix sum over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int other = __shfl_up(value, d, 64); if (lane >= d) value += other; }
    return value;
}

__global__ void __launch_bounds__(64) k_jpeg_entropy(const int16_t* __restrict__ coefficients, uint8_t* __restrict__ segments, uint32_t* __restrict__ lengths,
                                                     JpegTables tables, JpegGeometry g) {
    __shared__ uint32_t huffman[2*272];
    __shared__ uint32_t bits[JPEG_BIT_WORDS];
    __shared__ __attribute__((aligned(16))) uint8_t stage[JPEG_STAGE_BYTES];
    const int lane = threadIdx.x;
    const size_t interval = (size_t)blockIdx.z*g.mcus_y + blockIdx.x;
    const int16_t* block = coefficients + interval*g.mcus_x*384;
    uint8_t* segment = segments + interval*(size_t)g.segment_capacity;
    for (int k = lane; k < 2*272; k += 64) huffman[k] = tables.huffman[k];
    bits[lane] = 0;
    __syncthreads();

    int predictor[3] = {0, 0, 0};
    int carry = 0;                                                  // bits of the buffer's first byte that are already taken (0…7)
    int staged = 0, written = 0;                                    // bytes in the stage; bytes of the segment already stored
    bool overflow = false;
    const int blocks = g.mcus_x*6;
    for (int n = 0; n <= blocks; n++) {
        int total;                                                  // bits in the buffer after this step
        if (n < blocks) {
            const int b = n % 6, component = b < 4 ? 0 : b - 3;
            const uint32_t* table = huffman + (component ? 272 : 0);
            int value = block[(size_t)n*64 + lane];
            const int dc = __shfl(value, 0, 64);
            if (lane == 0) value = dc - predictor[component];
            predictor[component] = dc;
            const unsigned long long nonzero = __ballot(lane > 0 && value != 0);
            const int magnitude = abs(value);
            const int size = magnitude ? 32 - __clz(magnitude) : 0;
            const unsigned long long extra = (unsigned long long)((value < 0 ? value - 1 : value) & ((1 << size) - 1));
            unsigned long long code = 0;
            int length = 0;
            if (lane == 0) {
                const uint32_t entry = table[size];
                code = ((unsigned long long)(entry & 0xffffu) << size) | extra;
                length = (int)(entry >> 16) + size;
            } else if (value != 0) {
                const unsigned long long before = nonzero & ((1ull << lane) - 1ull);
                const int previous = before ? 63 - __clzll((long long)before) : 0;
                const int run = lane - 1 - previous;
                const uint32_t zrl = table[16 + 0xf0], entry = table[16 + ((run & 15) << 4) + size];
                for (int k = 0; k < (run >> 4); k++) { code = (code << (zrl >> 16)) | (zrl & 0xffffu); length += (int)(zrl >> 16); }
                code = (((code << (entry >> 16)) | (entry & 0xffffu)) << size) | extra;
                length += (int)(entry >> 16) + size;
            } else if (lane == 63) {                                 // the block ends in zeros: EOB, in the last lane's place
                const uint32_t entry = table[16];
                code = entry & 0xffffu; length = (int)(entry >> 16);
            }
            const int end = jpeg_wave_scan(length, lane);
            if (length) {
                const int offset = carry + end - length, word = offset >> 5, top = (offset & 31) + length;   // top ≤ 31 + 59
                if (top <= 64) {
                    const unsigned long long high = code << (64 - top);
                    atomicOr(&bits[word], (uint32_t)(high >> 32));
                    if ((uint32_t)high) atomicOr(&bits[word + 1], (uint32_t)high);
                } else {
                    const unsigned long long high = code >> (top - 64);
                    atomicOr(&bits[word], (uint32_t)(high >> 32));
                    atomicOr(&bits[word + 1], (uint32_t)high);
                    atomicOr(&bits[word + 2], (uint32_t)(code << (96 - top)));
                }
            }
            total = carry + __shfl(end, 63, 64);
        } else {                                                    // the interval's end: the last byte is completed with ones
            total = carry;
            if (carry && lane == 0) bits[0] |= 0xffffffffu >> carry & 0xff000000u;
            if (carry) total = 8;
        }
        __syncthreads();
        // whole bytes → the stage, with a zero byte behind every FF
        const int whole = total >> 3;
        for (int first = 0; first < whole; first += 64) {
            const int i = first + lane;
            const int byte = i < whole ? (int)((bits[i >> 2] >> (24 - 8*(i & 3))) & 0xffu) : 0;
            const unsigned long long full = __ballot(byte == 0xff);
            const int at = staged + lane + __popcll(full & ((1ull << lane) - 1ull));
            if (i < whole) { stage[at] = (uint8_t)byte; if (byte == 0xff) stage[at + 1] = 0; }
            staged += min(64, whole - first) + __popcll(full);
        }
        const uint32_t left = (total & 7) ? (bits[whole >> 2] >> (24 - 8*(whole & 3))) & 0xffu : 0u;
        __syncthreads();
        bits[lane] = lane == 0 ? left << 24 : 0u;
        carry = total & 7;
        // the stage → the segment
        const bool last = n == blocks;
        while (staged >= JPEG_STAGE_FLUSH || (last && staged > 0)) {
            const int chunk = min(staged, JPEG_STAGE_FLUSH);
            if (written + chunk > g.segment_capacity) overflow = true;
            if (!overflow && lane*16 < chunk) *(uint4*)(segment + written + lane*16) = *(const uint4*)(stage + lane*16);   // (the last store may carry up to 15 bytes past the length: inside the capacity, a multiple of 16)
            __syncthreads();
            uint8_t moved[8];
            const int rest = staged - chunk;                        // ≤ 512
#pragma unroll
            for (int k = 0; k < 8; k++) moved[k] = lane + 64*k < rest ? stage[chunk + lane + 64*k] : 0;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; k++) if (lane + 64*k < rest) stage[lane + 64*k] = moved[k];
            written += chunk; staged = rest;
        }
        __syncthreads();
    }
    if (lane == 0) lengths[interval] = overflow ? JPEG_OVERFLOW : (uint32_t)written;
}

// ---- 3. header, segments, markers → the sink frame ---------------------------------------------------------------------------------
// One block per interval: it sums the lengths in front of its own (and learns whether any interval overflowed), copies its segment
// to its place, puts RSTn behind it — or, the last one, EOI and the sink frame's header; block 0 copies the constant header too.
__global__ void __launch_bounds__(256) k_jpeg_pack(const uint8_t* __restrict__ segments, const uint32_t* __restrict__ lengths, uint8_t* __restrict__ sink, size_t sink_stride,
                                                   JpegTables tables, JpegGeometry g) {
    __shared__ unsigned long long partial[256];
    __shared__ int any_overflow;
    const int t = threadIdx.x, row = blockIdx.x;
    const uint32_t* frame_lengths = lengths + (size_t)blockIdx.z*g.mcus_y;
    uint8_t* frame = sink + (size_t)blockIdx.z*sink_stride;
    uint8_t* payload = frame + JPEG_SINK_HEADER;
    if (t == 0) any_overflow = 0;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    bool bad = false;
    for (int k = t; k < g.mcus_y; k += 256) {
        const uint32_t n = frame_lengths[k];
        if (n == JPEG_OVERFLOW) bad = true;
        else { all += n; if (k < row) before += n; }
    }
    if (bad) any_overflow = 1;
    partial[t] = before;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) { if (t < d) partial[t] += partial[t + d]; __syncthreads(); }
    before = partial[0];
    __syncthreads();
    partial[t] = all;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) { if (t < d) partial[t] += partial[t + d]; __syncthreads(); }
    all = partial[0];
    const unsigned long long total = (unsigned long long)tables.header_bytes + all + 2ull*(g.mcus_y - 1) + 2ull;
    const bool fits = !any_overflow && total <= (unsigned long long)g.payload_capacity;
    const bool final_row = row == g.mcus_y - 1;
    if (fits) {
        if (row == 0) for (int k = t; k < tables.header_bytes; k += 256) payload[k] = tables.header[k];
        const uint32_t mine = frame_lengths[row];
        uint8_t* out = payload + tables.header_bytes + before + 2ull*row;
        const uint8_t* in = segments + ((size_t)blockIdx.z*g.mcus_y + row)*(size_t)g.segment_capacity;
        for (uint32_t k = t; k < mine; k += 256) out[k] = in[k];
        if (t == 0) { out[mine] = 0xff; out[mine + 1] = final_row ? 0xd9 : (uint8_t)(0xd0 + (row & 7)); }
    }
    if (final_row && t < JPEG_SINK_HEADER/4)
        ((uint32_t*)frame)[t] = t == 0 ? JPEG_SINK_MAGIC : t == 1 ? (fits ? (uint32_t)total : 0u) : t == 2 ? (fits ? 0u : 1u) : 0u;
}

}  // namespace sf
