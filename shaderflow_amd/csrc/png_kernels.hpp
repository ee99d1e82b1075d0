// png_kernels.hpp — lossless PNG of RGB8 frames on the device (capi_png.hip launches these).
//
// The stream is DEFINED here, like the JPEG stream (jpeg_kernels.hpp), and restated byte for byte by tests/png_ref.py:
//   * picture: signature, IHDR (width, height, bit depth 8, colour type 2, compression 0, filter 0, interlace 0), one IDAT chunk per
//     stripe, IEND. Rows go top first (`bottom_up`: the frame's rows are stored bottom-up and are read in reverse);
//   * filter, bpp = 3: every row gets the type of None, Sub, Up, Average, Paeth whose filtered bytes, read as signed, have the smallest
//     sum of absolute values, ties to the lowest type. The row above is the raw previous row (also across stripes), zeros above row 0;
//   * stripes: the filtered stream (rows of 1 + 3W bytes) is cut every 8 rows; a stripe is one deflate block in one IDAT chunk of its
//     own. The first chunk starts with the zlib header 78 01. Every stripe but the last ends with an empty stored block (three zero
//     bits, zero bits to the byte boundary, 00 00 FF FF), so the next one starts on a byte; the last block has BFINAL = 1, is padded
//     with zero bits to a byte and is followed, in its chunk, by the Adler-32 of the whole filtered stream, big-endian;
//   * parse: greedy, literals and matches of distance 1. Where a byte repeats the byte before it in the same stripe and at least 3
//     such bytes follow each other, a match takes up to 258 of them (what zlib's Z_RLE strategy takes); nothing reaches back across
//     a stripe boundary;
//   * codes: a histogram of 286 literal/length symbols (end-of-block counted once) and 30 distance symbols gives the stripe's own
//     codes (BTYPE = 10), at most 15 bits, and the code-length code over the 316 lengths, at most 7 bits. One alphabet's lengths:
//       - while fewer than two symbols have a count, the lowest-numbered symbol without one gets the count 1 (every code is complete);
//       - the two nodes with the smallest (weight, index) are merged until one is left: a leaf's index is its symbol, the k-th node
//         made has index n + k; a symbol's length is its depth;
//       - while the deepest symbol is deeper than the limit, every count w > 0 becomes (w + 1) >> 1 and the tree is built again.
//     Codes are canonical (RFC 1951 3.2.2). The header always states HLIT = 286, HDIST = 30, HCLEN = 19 and writes each of the 316
//     lengths with the symbols 0…15 (no repeat symbols);
//   * fixed-block fallback: when the dynamic block, header included, is not strictly smaller in bits than the same parse under the
//     fixed codes (BTYPE = 01), the fixed codes are written. A literal then costs at most 9 bits and a match at most 18 for at least
//     3 bytes, so a stripe of n bytes takes at most ⌈9n/8⌉ + 16 bytes with its framing: a sink frame sized from that cannot overflow.
//
// Three kernels, grid.z = frames: k_png_filter (one block per row: filter choice, filtered row, the row's Adler partial sums),
// k_png_deflate (one wave per stripe: parse + histogram, code lengths, block header, parse + code, the chunk's CRC-32 as the bytes
// leave), k_png_pack (one block per stripe: chunk framing to its place, signature + IHDR, IEND and the sink frame's header).
// k_png_tables runs the code-length step alone on a caller's histogram (sfx_png_code_lengths).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sf {

constexpr uint32_t PNG_SINK_MAGIC = 0x504a4653u;                    // the sized ring's sink frame (jpeg_kernels.hpp JPEG_SINK_MAGIC)
constexpr int PNG_SINK_HEADER = 64;                                 // [magic, payload bytes, status, 0…] then the payload
constexpr int PNG_STRIPE_ROWS = 8;
constexpr int PNG_LITERALS = 286, PNG_DISTANCES = 30, PNG_SYMBOLS = 316, PNG_META = 19;
constexpr int PNG_HEAD_BYTES = 33;                                  // signature + IHDR chunk
constexpr uint32_t PNG_CRC_POLY = 0xedb88320u;
constexpr uint32_t PNG_ADLER_BASE = 65521u;
constexpr int PNG_FLUSH_BYTES = 1024;                               // the bit buffer leaves 1 KiB at a time, in 16-byte stores
constexpr int PNG_BIT_WORDS = 320;                                  // 1024 bytes + what one step adds at the most (64 x 25 bits) + a word
constexpr int PNG_WINDOW = 1024;                                    // bytes of a stripe a wave fetches at a time (one trip to memory)
constexpr int PNG_SHIFTS = 65;                                      // x^(128 k) mod P, k = 0…64

struct PngOrder { uint8_t of[PNG_META]; };
constexpr PngOrder PNG_ORDER = {{16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15}};

struct PngGeometry {
    int width, height;
    int row_bytes;                  // 1 + 3W
    int stripes;
    int segment_capacity;           // bytes a stripe's chunk data may take in the scratch (a multiple of 16)
    int payload_capacity;           // of a sink frame
    int bottom_up;
};

struct PngTables {
    const uint32_t* shift;          // [PNG_SHIFTS] x^(128 k) mod P in the CRC's reflected form (host-made)
    uint32_t idat_state;            // the CRC register behind "IDAT"
    uint8_t head[PNG_HEAD_BYTES + 3];
};

__device__ __forceinline__ int png_wave_sum(int value) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) value += __shfl_xor(value, d, 64);
    return value;
}
__device__ __forceinline__ unsigned long long png_wave_sum64(unsigned long long value) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) value += __shfl_xor(value, d, 64);
    return value;
}
__device__ __forceinline__ int png_wave_max(int value) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) value = max(value, __shfl_xor(value, d, 64));
    return value;
}
__device__ __forceinline__ int png_wave_min(int value) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) value = min(value, __shfl_xor(value, d, 64));
    return value;
}
__device__ __forceinline__ unsigned long long png_wave_min64(unsigned long long value) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const unsigned long long other = __shfl_xor(value, d, 64); value = other < value ? other : value; }
    return value;
}
__device__ __forceinline__ uint32_t png_wave_xor(uint32_t value) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) value ^= (uint32_t)__shfl_xor((int)value, d, 64);
    return value;
}

// ---- 1. row filters ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int png_filtered(int type, int v, int a, int b, int c) {
    int predictor = 0;
    if (type == 1) predictor = a;
    else if (type == 2) predictor = b;
    else if (type == 3) predictor = (a + b) >> 1;
    else if (type == 4) {
        const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2*c);
        predictor = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    }
    return (v - predictor) & 0xff;
}

// One block of 256 threads per row: the five candidates' sums, the choice, the filtered row behind its type byte, and the row's share
// of the Adler-32: sums[row] = {Σ d mod 65521, Σ (L - k) d[k] mod 65521} over the row's L = 1 + 3W bytes d
__global__ void __launch_bounds__(256) k_png_filter(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ filtered, uint32_t* __restrict__ sums, PngGeometry g) {
    __shared__ uint32_t cost[4][5];
    __shared__ unsigned long long adler[4][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, y = blockIdx.x, n = g.row_bytes - 1;
    const uint8_t* frame = rgb + (size_t)blockIdx.z*g.height*n;
    const uint8_t* row = frame + (size_t)(g.bottom_up ? g.height - 1 - y : y)*n;
    const uint8_t* above = y ? frame + (size_t)(g.bottom_up ? g.height - y : y - 1)*n : row;   // (not read when y == 0)
    int sum[5] = {0, 0, 0, 0, 0};
    for (int x = t; x < n; x += 256) {
        const int v = row[x], a = x >= 3 ? row[x - 3] : 0, b = y ? above[x] : 0, c = (y && x >= 3) ? above[x - 3] : 0;
#pragma unroll
        for (int k = 0; k < 5; k++) { const int f = png_filtered(k, v, a, b, c); sum[k] += f < 128 ? f : 256 - f; }
    }
#pragma unroll
    for (int k = 0; k < 5; k++) { const int total = png_wave_sum(sum[k]); if (lane == 0) cost[wave][k] = (uint32_t)total; }
    __syncthreads();
    int type = 0;
    uint32_t best = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < 5; k++) { const uint32_t total = cost[0][k] + cost[1][k] + cost[2][k] + cost[3][k]; if (total < best) { best = total; type = k; } }
    uint8_t* out = filtered + ((size_t)blockIdx.z*g.height + y)*g.row_bytes;
    unsigned long long s1 = 0, s2 = 0;
    if (t == 0) { out[0] = (uint8_t)type; s1 = (unsigned long long)type; s2 = (unsigned long long)type*g.row_bytes; }
    for (int x = t; x < n; x += 256) {
        const int v = row[x], a = x >= 3 ? row[x - 3] : 0, b = y ? above[x] : 0, c = (y && x >= 3) ? above[x - 3] : 0;
        const int f = png_filtered(type, v, a, b, c);
        out[1 + x] = (uint8_t)f;
        s1 += (unsigned long long)f; s2 += (unsigned long long)f*(unsigned long long)(n - x);
    }
    s1 = png_wave_sum64(s1); s2 = png_wave_sum64(s2);
    if (lane == 0) { adler[wave][0] = s1; adler[wave][1] = s2; }
    __syncthreads();
    if (t < 2) sums[(((size_t)blockIdx.z*g.height + y) << 1) + t] = (uint32_t)((adler[0][t] + adler[1][t] + adler[2][t] + adler[3][t]) % PNG_ADLER_BASE);
}

// ---- 2. one stripe per wave: parse, histogram, codes, bits, CRC --------------------------------------------------------------------
struct PngWork {                    // the LDS of a wave
    uint32_t histogram[PNG_SYMBOLS];
    uint32_t scaled[PNG_LITERALS];
    uint32_t weight[2*PNG_LITERALS];
    uint16_t parent[2*PNG_LITERALS];
    uint32_t meta_count[PNG_META];
    uint32_t first_code[16];
    uint32_t table[PNG_SYMBOLS];    // (length << 16) | the code, bit-reversed
    uint32_t meta_table[PNG_META];
    uint32_t crc[256];
    uint8_t lengths[PNG_SYMBOLS];
    uint8_t meta_lengths[PNG_META + 1];
    __attribute__((aligned(16))) uint32_t bits[PNG_BIT_WORDS];
    uint8_t window[PNG_WINDOW + 64];   // a piece of the stripe, from one byte in front of it to two behind it
};

// Code lengths of one alphabet of n symbols (the header states the rule): counts → out, both in LDS
__device__ void png_code_lengths(PngWork& w, const uint32_t* counts, int n, int limit, uint8_t* out, int lane) {
    for (int s = lane; s < n; s += 64) w.scaled[s] = counts[s];
    __syncthreads();
    int used;
    for (;;) {
        int mine = 0, free_symbol = n;
        for (int s = lane; s < n; s += 64) { if (w.scaled[s]) mine++; else free_symbol = min(free_symbol, s); }
        used = png_wave_sum(mine);
        if (used >= 2) break;
        free_symbol = png_wave_min(free_symbol);
        if (lane == 0) w.scaled[free_symbol] = 1;
        __syncthreads();
    }
    for (;;) {
        for (int s = lane; s < n; s += 64) w.weight[s] = w.scaled[s];
        __syncthreads();
        int made = n;
        for (int k = 0; k < used - 1; k++) {
            unsigned long long first = ~0ull, second = ~0ull;
            for (int i = lane; i < made; i += 64) {
                const uint32_t weight = w.weight[i];
                if (weight) {
                    const unsigned long long key = ((unsigned long long)weight << 32) | (uint32_t)i;
                    if (key < first) { second = first; first = key; } else if (key < second) second = key;
                }
            }
            const unsigned long long least = png_wave_min64(first);
            const unsigned long long next = png_wave_min64(first == least ? second : first);
            if (lane == 0) {
                const uint32_t i1 = (uint32_t)least, i2 = (uint32_t)next;
                w.weight[made] = (uint32_t)(least >> 32) + (uint32_t)(next >> 32);
                w.weight[i1] = 0; w.weight[i2] = 0;
                w.parent[i1] = (uint16_t)made; w.parent[i2] = (uint16_t)made;
            }
            made++;
            __syncthreads();
        }
        const int root = made - 1;
        int deepest = 0;
        for (int s = lane; s < n; s += 64) {
            int depth = 0;
            if (w.scaled[s]) for (int node = s; node != root; node = w.parent[node]) depth++;
            out[s] = (uint8_t)depth;
            deepest = max(deepest, depth);
        }
        deepest = png_wave_max(deepest);
        __syncthreads();
        if (deepest <= limit) break;
        for (int s = lane; s < n; s += 64) if (w.scaled[s]) w.scaled[s] = (w.scaled[s] + 1) >> 1;
        __syncthreads();
    }
}

__device__ __forceinline__ int png_fixed_length(int s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < PNG_LITERALS ? 8 : 5; }
__device__ __forceinline__ int png_extra_bits(int s) { return (s >= 265 && s < 285) ? (s - 261) >> 2 : 0; }

// The tables step on w.histogram: w.lengths (the dynamic code's), w.meta_lengths; → whether the block takes the fixed codes
__device__ bool png_tables(PngWork& w, int lane) {
    png_code_lengths(w, w.histogram, PNG_LITERALS, 15, w.lengths, lane);
    png_code_lengths(w, w.histogram + PNG_LITERALS, PNG_DISTANCES, 15, w.lengths + PNG_LITERALS, lane);
    if (lane < PNG_META) w.meta_count[lane] = 0;
    __syncthreads();
    for (int s = lane; s < PNG_SYMBOLS; s += 64) atomicAdd(&w.meta_count[w.lengths[s]], 1u);
    __syncthreads();
    png_code_lengths(w, w.meta_count, PNG_META, 7, w.meta_lengths, lane);
    int dynamic = 0, fixed = 0;
    for (int s = lane; s < PNG_SYMBOLS; s += 64) {
        const int length = w.lengths[s], count = (int)w.histogram[s], extra = count*png_extra_bits(s);
        dynamic += w.meta_lengths[length] + count*length + extra;
        fixed += count*png_fixed_length(s) + extra;
    }
    dynamic = 3 + 14 + 3*PNG_META + png_wave_sum(dynamic);
    fixed = 3 + png_wave_sum(fixed);
    return !(dynamic < fixed);
}

// canonical codes of n lengths → (length << 16) | reversed code; lane L owns the codes of length L
__device__ void png_canonical(PngWork& w, const uint8_t* lengths, int n, uint32_t* table, int lane) {
    if (lane < 16) {
        uint32_t count = 0;
        if (lane) for (int s = 0; s < n; s++) count += lengths[s] == lane;
        w.first_code[lane] = count;
    }
    __syncthreads();
    if (lane == 0) {
        uint32_t code = 0, before = 0;
        for (int bits = 1; bits < 16; bits++) { code = (code + before) << 1; before = w.first_code[bits]; w.first_code[bits] = code; }
    }
    __syncthreads();
    if (lane == 0) { for (int s = 0; s < n; s++) if (!lengths[s]) table[s] = 0; }
    else if (lane < 16) {
        uint32_t code = w.first_code[lane];
        for (int s = 0; s < n; s++) if (lengths[s] == lane) table[s] = ((uint32_t)lane << 16) | (__brev(code++) >> (32 - lane));
    }
    __syncthreads();
}

// A match length 3…258 → its symbol; the extra bits are png_extra_bits(symbol), their value (length - 3) & mask
__device__ __forceinline__ int png_length_symbol(int length) {
    if (length == 258) return 285;
    const int n = length - 3;
    if (n < 8) return 257 + n;
    const int extra = 29 - __clz(n);
    return 261 + 4*extra + ((n >> extra) & 3);
}

// The stripe's bytes first - 1 … first + PNG_WINDOW + 1 → w.window (zeros outside the stripe), every lane's loads in flight together
__device__ __forceinline__ void png_load_window(PngWork& w, const uint8_t* __restrict__ data, int n, int first, int lane) {
    constexpr int TRIPS = (PNG_WINDOW + 3 + 63)/64;
    uint8_t fetched[TRIPS];
#pragma unroll
    for (int k = 0; k < TRIPS; k++) { const int i = first - 1 + k*64 + lane; fetched[k] = (i >= 0 && i < n) ? data[i] : (uint8_t)0; }
    __syncthreads();                                                // (the window's last readers are through)
#pragma unroll
    for (int k = 0; k < TRIPS; k++) w.window[k*64 + lane] = fetched[k];
    __syncthreads();
}

// What position base + lane of the stripe contributes: -1 nothing, 0…255 a literal, 256 + length a match (said at the match's last
// byte: tokens do not overlap, so their order by end is their order by start). `start`: the last position whose byte differs from the
// byte before it, carried from step to step; r counts the repeats of the current run in chunks of 258.
// `window`: the stripe's bytes from position base - 1 on, in LDS (png_load_window).
__device__ __forceinline__ int png_token(const uint8_t* window, int n, int base, int lane, int& start) {
    const int i = base + lane;
    const bool inside = i < n;
    const int c = inside ? window[lane + 1] : -1, p = (inside && i > 0) ? window[lane] : -2;
    const bool repeat = c == p;
    const int c1 = (inside && i + 1 < n) ? window[lane + 2] : -3, c2 = (inside && i + 2 < n) ? window[lane + 3] : -4;
    const bool next_repeats = c1 == c, second_repeats = c2 == c1;
    const unsigned long long heads = __ballot(!repeat);
    const unsigned long long before = heads & (~0ull >> (63 - lane));
    const int head = before ? base + 63 - __clzll((long long)before) : start;
    if (heads) start = base + 63 - __clzll((long long)heads);
    if (!inside) return -1;
    if (!repeat) return c;
    const int r = (i - head - 1) % 258;
    if (r == 257) return 256 + 258;
    if (!next_repeats) return r + 1 >= 3 ? 256 + r + 1 : c;
    if (r == 0 && !second_repeats) return c;
    return -1;
}

// `bits` bits of `value` per lane, LSB first, behind the `position` bits the buffer holds
__device__ __forceinline__ void png_emit(uint32_t* buffer, unsigned long long value, int bits, int& position, int lane) {
    // the prefix sum of 64 counts below 64, bit plane by bit plane: six ballots and mbcnt, no trip through the LDS crossbar
    int before = 0, total = 0;
#pragma unroll
    for (int plane = 0; plane < 6; plane++) {
        const unsigned long long set = __ballot((bits >> plane) & 1);
        before += (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(set >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)set, 0u)) << plane;
        total += __popcll(set) << plane;
    }
    if (bits) {
        const int offset = position + before;
        const unsigned long long shifted = value << (offset & 31);                       // ≤ 32 + 31 bits
        atomicOr(&buffer[offset >> 5], (uint32_t)shifted);
        if (shifted >> 32) atomicOr(&buffer[(offset >> 5) + 1], (uint32_t)(shifted >> 32));
    }
    position += total;
    __syncthreads();
}

__device__ __forceinline__ uint32_t png_gf_multiply(uint32_t a, uint32_t b) {          // a·b mod P, reflected: x^0 is bit 31
    uint32_t product = 0;
#pragma unroll 4
    for (int k = 0; k < 32; k++) {
        if (a & 0x80000000u) product ^= b;
        a <<= 1;
        b = (b >> 1) ^ ((b & 1u) ? PNG_CRC_POLY : 0u);
    }
    return product;
}

// Whole bytes of the bit buffer → the segment, 1 KiB at a time (`all`: everything, the buffer then holds whole bytes only). The CRC
// register takes them as they leave: a lane the raw CRC of its 16 bytes, times x^(128·blocks behind it); the tail bytewise.
__device__ void png_drain(PngWork& w, uint8_t* __restrict__ segment, int capacity, int& written, int& position, uint32_t& crc, bool& overflow,
                          const uint32_t* __restrict__ shift, bool all, int lane) {
    while (position >= 8*PNG_FLUSH_BYTES || (all && position > 0)) {
        const int bytes = min(position >> 3, PNG_FLUSH_BYTES), blocks = bytes >> 4, tail = bytes & 15;
        const bool mine = lane*16 < bytes;
        const uint4 value = mine ? ((const uint4*)w.bits)[lane] : make_uint4(0, 0, 0, 0);
        if (written + ((bytes + 15) & ~15) > capacity) overflow = true;
        if (mine && !overflow) *(uint4*)(segment + written + lane*16) = value;            // (the last store may carry up to 15 bytes past the length: inside the capacity)
        uint32_t part = 0;
        if (lane < blocks) {
            const uint32_t words[4] = {value.x, value.y, value.z, value.w};
            uint32_t c = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) c = w.crc[(c ^ (words[k >> 2] >> (8*(k & 3)))) & 0xffu] ^ (c >> 8);
            part = png_gf_multiply(c, shift[blocks - 1 - lane]);
        }
        crc = png_gf_multiply(crc, shift[blocks]) ^ png_wave_xor(part);
        for (int k = blocks*16; k < blocks*16 + tail; k++) crc = w.crc[(crc ^ (w.bits[k >> 2] >> (8*(k & 3)))) & 0xffu] ^ (crc >> 8);
        const uint32_t moved = w.bits[PNG_FLUSH_BYTES/4 + lane];                          // PNG_BIT_WORDS = 1 KiB + 64 words
        __syncthreads();
        for (int k = lane; k < PNG_BIT_WORDS; k += 64) w.bits[k] = 0;
        __syncthreads();
        if (bytes == PNG_FLUSH_BYTES) w.bits[lane] = moved;
        __syncthreads();
        written += bytes; position -= 8*bytes;
    }
}

__global__ void __launch_bounds__(64) k_png_deflate(const uint8_t* __restrict__ filtered, const uint32_t* __restrict__ sums, uint8_t* __restrict__ segments,
                                                    uint32_t* __restrict__ lengths, uint32_t* __restrict__ crcs, PngTables tables, PngGeometry g) {
    __shared__ PngWork w;
    const int lane = threadIdx.x, stripe = blockIdx.x;
    const size_t index = (size_t)blockIdx.z*g.stripes + stripe;
    const int rows = min(PNG_STRIPE_ROWS, g.height - stripe*PNG_STRIPE_ROWS), n = rows*g.row_bytes;
    const uint8_t* data = filtered + ((size_t)blockIdx.z*g.height + (size_t)stripe*PNG_STRIPE_ROWS)*g.row_bytes;
    uint8_t* segment = segments + index*(size_t)g.segment_capacity;
    const bool last = stripe == g.stripes - 1;

    for (int k = lane; k < PNG_SYMBOLS; k += 64) w.histogram[k] = 0;
    for (int k = lane; k < PNG_BIT_WORDS; k += 64) w.bits[k] = 0;
    for (int k = lane; k < 256; k += 64) {
        uint32_t c = (uint32_t)k;
#pragma unroll
        for (int bit = 0; bit < 8; bit++) c = (c >> 1) ^ ((c & 1u) ? PNG_CRC_POLY : 0u);
        w.crc[k] = c;
    }
    __syncthreads();

    // the parse, first time: the histogram
    int start = 0;
    for (int first = 0; first < n; first += PNG_WINDOW) {
        png_load_window(w, data, n, first, lane);
        const int stop = min(n, first + PNG_WINDOW);
        for (int base = first; base < stop; base += 64) {
            const int token = png_token(w.window + (base - first), n, base, lane, start);
            // (filtered shader frames are mostly 0, 1 and 255: those are counted by ballot, not by 64 atomics on one word)
            const unsigned long long zeros = __ballot(token == 0), ones = __ballot(token == 1), minus = __ballot(token == 255);
            if (token >= 256) { atomicAdd(&w.histogram[png_length_symbol(token - 256)], 1u); atomicAdd(&w.histogram[PNG_LITERALS], 1u); }
            else if (token > 1 && token != 255) atomicAdd(&w.histogram[token], 1u);
            if (lane == 0) { w.histogram[0] += (uint32_t)__popcll(zeros); w.histogram[1] += (uint32_t)__popcll(ones); w.histogram[255] += (uint32_t)__popcll(minus); }
        }
    }
    if (lane == 0) atomicAdd(&w.histogram[256], 1u);
    __syncthreads();

    const bool fixed = png_tables(w, lane);
    int position = 0, written = 0;
    uint32_t crc = tables.idat_state;
    bool overflow = false;
    if (stripe == 0) { if (lane == 0) w.bits[0] = 0x0178u; position = 16; }
    __syncthreads();
    if (fixed) {
        for (int s = lane; s < PNG_SYMBOLS; s += 64) {
            const int length = png_fixed_length(s);
            const uint32_t code = s < 144 ? 0x30u + s : s < 256 ? 0x190u + (s - 144) : s < 280 ? (uint32_t)(s - 256) : s < PNG_LITERALS ? 0xc0u + (s - 280) : (uint32_t)(s - PNG_LITERALS);
            w.table[s] = ((uint32_t)length << 16) | (__brev(code) >> (32 - length));
        }
        __syncthreads();
        png_emit(w.bits, (last ? 1u : 0u) | (1u << 1), lane == 0 ? 3 : 0, position, lane);
    } else {
        png_canonical(w, w.lengths, PNG_LITERALS, w.table, lane);
        png_canonical(w, w.lengths + PNG_LITERALS, PNG_DISTANCES, w.table + PNG_LITERALS, lane);
        png_canonical(w, w.meta_lengths, PNG_META, w.meta_table, lane);
        for (int first = 0; first < 1 + PNG_META + PNG_SYMBOLS; first += 64) {
            const int item = first + lane;
            uint32_t value = 0; int bits = 0;
            if (item == 0) { value = (last ? 1u : 0u) | (2u << 1) | ((PNG_LITERALS - 257) << 3) | ((PNG_DISTANCES - 1) << 8) | ((PNG_META - 4) << 13); bits = 17; }
            else if (item <= PNG_META) { value = w.meta_lengths[PNG_ORDER.of[item - 1]]; bits = 3; }
            else if (item < 1 + PNG_META + PNG_SYMBOLS) { const uint32_t entry = w.meta_table[w.lengths[item - 1 - PNG_META]]; value = entry & 0xffffu; bits = (int)(entry >> 16); }
            png_emit(w.bits, value, bits, position, lane);
        }
    }

    // the parse, second time: the codes
    start = 0;
    for (int first = 0; first < n; first += PNG_WINDOW) {
      png_load_window(w, data, n, first, lane);
      const int stop = min(n, first + PNG_WINDOW);
      for (int base = first; base < stop; base += 64) {
        const int token = png_token(w.window + (base - first), n, base, lane, start);
        unsigned long long value = 0; int bits = 0;
        if (token >= 256) {
            const int length = token - 256, symbol = png_length_symbol(length), extra = png_extra_bits(symbol);
            const uint32_t entry = w.table[symbol], distance = w.table[PNG_LITERALS];
            bits = (int)(entry >> 16);
            value = (entry & 0xffffu) | ((unsigned long long)((length - 3) & ((1 << extra) - 1)) << bits);
            bits += extra;
            value |= (unsigned long long)(distance & 0xffffu) << bits;
            bits += (int)(distance >> 16);
        } else if (token >= 0) { const uint32_t entry = w.table[token]; value = entry & 0xffffu; bits = (int)(entry >> 16); }
        png_emit(w.bits, value, bits, position, lane);
        png_drain(w, segment, g.segment_capacity, written, position, crc, overflow, tables.shift, false, lane);
      }
    }
    png_emit(w.bits, w.table[256] & 0xffffu, lane == 0 ? (int)(w.table[256] >> 16) : 0, position, lane);
    uint32_t trailer = 0xffff0000u;                                 // LEN = 0, NLEN = FFFF of the empty stored block
    if (last) {
        unsigned long long s1 = 0, s2 = 0, s3 = 0;                  // Σ a, Σ b, Σ a·(rows behind) over the rows' partial sums
        const uint32_t* row_sums = sums + (((size_t)blockIdx.z*g.height) << 1);
        for (int y = lane; y < g.height; y += 64) { const unsigned long long a = row_sums[2*y]; s1 += a; s2 += row_sums[2*y + 1]; s3 += a*(unsigned long long)(g.height - 1 - y); }
        s1 = png_wave_sum64(s1) % PNG_ADLER_BASE; s2 = png_wave_sum64(s2) % PNG_ADLER_BASE; s3 = png_wave_sum64(s3) % PNG_ADLER_BASE;
        const unsigned long long a = (1 + s1) % PNG_ADLER_BASE;
        const unsigned long long b = (s2 + ((unsigned long long)g.row_bytes % PNG_ADLER_BASE)*(((unsigned long long)g.height + s3) % PNG_ADLER_BASE)) % PNG_ADLER_BASE;
        const uint32_t adler = (uint32_t)((b << 16) | a);
        trailer = ((adler & 0xffu) << 24) | ((adler & 0xff00u) << 8) | ((adler >> 8) & 0xff00u) | (adler >> 24);
        position = (position + 7) & ~7;
    } else position = (position + 3 + 7) & ~7;
    png_emit(w.bits, trailer, lane == 0 ? 32 : 0, position, lane);
    png_drain(w, segment, g.segment_capacity, written, position, crc, overflow, tables.shift, true, lane);
    if (lane == 0) { lengths[index] = overflow ? 0xffffffffu : (uint32_t)written; crcs[index] = ~crc; }
}

// the tables step alone, on a caller's histogram (sfx_png_code_lengths)
__global__ void __launch_bounds__(64) k_png_tables(const uint32_t* __restrict__ histogram, uint8_t* __restrict__ lengths, int* __restrict__ fixed) {
    __shared__ PngWork w;
    const int lane = threadIdx.x;
    for (int k = lane; k < PNG_SYMBOLS; k += 64) w.histogram[k] = histogram[k];
    __syncthreads();
    const bool takes_fixed = png_tables(w, lane);
    __syncthreads();
    for (int k = lane; k < PNG_SYMBOLS; k += 64) lengths[k] = w.lengths[k];
    if (lane == 0) *fixed = takes_fixed ? 1 : 0;
}

// ---- 3. chunks → the sink frame ----------------------------------------------------------------------------------------------------
// One block per stripe: it sums the chunks in front of its own, writes length, "IDAT", data and CRC to their place; block 0 the
// signature and IHDR too, the last block IEND and the sink frame's header (magic, payload bytes, status 0).
__global__ void __launch_bounds__(256) k_png_pack(const uint8_t* __restrict__ segments, const uint32_t* __restrict__ lengths, const uint32_t* __restrict__ crcs,
                                                  uint8_t* __restrict__ sink, size_t sink_stride, PngTables tables, PngGeometry g) {
    __shared__ unsigned long long partial[256];
    __shared__ int any_overflow;
    const int t = threadIdx.x, stripe = blockIdx.x;
    const size_t first = (size_t)blockIdx.z*g.stripes;
    uint8_t* frame = sink + (size_t)blockIdx.z*sink_stride;
    uint8_t* payload = frame + PNG_SINK_HEADER;
    if (t == 0) any_overflow = 0;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    bool bad = false;
    for (int k = t; k < g.stripes; k += 256) {
        const uint32_t n = lengths[first + k];
        if (n == 0xffffffffu) bad = true;
        else { all += n + 12ull; if (k < stripe) before += n + 12ull; }
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
    const unsigned long long total = (unsigned long long)PNG_HEAD_BYTES + all + 12ull;
    const bool fits = !any_overflow && total <= (unsigned long long)g.payload_capacity;
    const bool final_stripe = stripe == g.stripes - 1;
    if (fits) {
        if (stripe == 0 && t < PNG_HEAD_BYTES) payload[t] = tables.head[t];
        const uint32_t mine = lengths[first + stripe], crc = crcs[first + stripe];
        uint8_t* out = payload + PNG_HEAD_BYTES + before;
        const uint8_t* in = segments + (first + stripe)*(size_t)g.segment_capacity;
        for (uint32_t k = t; k < mine; k += 256) out[8 + k] = in[k];
        if (t < 4) { out[t] = (uint8_t)(mine >> (24 - 8*t)); out[8 + mine + t] = (uint8_t)(crc >> (24 - 8*t)); }
        if (t == 4) { out[4] = 'I'; out[5] = 'D'; out[6] = 'A'; out[7] = 'T'; }
        if (final_stripe && t == 5) {
            uint8_t* end = out + 12 + mine;
            const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
#pragma unroll
            for (int k = 0; k < 12; k++) end[k] = iend[k];
        }
    }
    if (final_stripe && t < PNG_SINK_HEADER/4)
        ((uint32_t*)frame)[t] = t == 0 ? PNG_SINK_MAGIC : t == 1 ? (fits ? (uint32_t)total : 0u) : t == 2 ? (fits ? 0u : 1u) : 0u;
}

}  // namespace sf
