// png_decode_kernels.hpp — PNG frames decoded where the texture lives: the counterpart of png_kernels.hpp. This comment is the
// normative text of the decode; tests/png_decode_ref.py restates it in Python, include/shaderflow_hip.h has the staged frame
// (sfx_png_frame: the record, one word per segment — where each IDAT chunk's bytes start in the payload — and the payload: the IDAT
// data concatenated, without the zlib header and the Adler-32 trailer) and the status bits (SFX_PNG_*).
//
// What is decoded: 8-bit RGB (colour type 2), compression 0, filter method 0, no interlace; the host refuses everything else
// (pngsource.py). Chunk CRC-32s are not checked anywhere; the Adler-32 of the inflated stream is, here.
//
// 1. Inflate (RFC 1951), complete: stored, fixed and dynamic blocks, any number of them, the repeat symbols 16, 17 and 18 (across the
//    border between the literal/length and the distance lengths too), any HLIT ≤ 286, HDIST ≤ 30 and HCLEN, codes up to 15 bits,
//    distances up to 32 768, overlapping matches. A code-length set that is over-subscribed is an error at the header; an incomplete
//    one (the single one-bit distance code, or any other) is an error only when a code that was not assigned is met. The output must
//    be exactly height x (1 + 3 width) bytes: a symbol that would write past that is refused before it writes.
//
//    One wave decodes: every lane runs the symbol loop on the same bits (the state is the wave's, not a lane's), and the lanes share
//    the copying of a match or a stored block and the building of the decode tables. The last 32 768 output bytes live in LDS (a ring);
//    matches read that ring, never global memory, and the ring is flushed to global memory 256 bytes at a time. A code's table in LDS:
//    `fast`, indexed by the next 10 bits, holds (symbol << 4 | length) for codes of up to 10 bits, 0xffff where a longer code begins
//    (those are decoded bit by bit against the canonical counts) and 0 where no code begins. Which error a bad tail is follows from
//    that look-up, zeros standing in behind the last bit: a code of up to 10 bits that is longer than what is left is
//    SFX_PNG_OUT_OF_BITS; where a longer code begins, bits are taken one by one, OUT_OF_BITS when they run out and SFX_PNG_BAD_CODE when
//    15 match none; where no code begins, OUT_OF_BITS with fewer than 10 bits left and BAD_CODE otherwise.
//
//    The bit reader takes bytes from [begin, end) of the payload and no others; every block consumes at least 3 bits and every symbol
//    at least 1, so the loops end with the payload's bits. Nothing is stored past `limit` output bytes.
//
//    Serial path (k_png_inflate_serial): one wave, the whole payload, from its first bit. Its errors are the frame's status. Bytes
//    between the last block and the trailer are SFX_PNG_BAD_ADLER (zlib would read the trailer from them).
//
//    Segment path: a wave per segment (IDAT chunk) decodes from the segment's first byte as if a block began there on a byte boundary
//    (k_png_inflate_count: no output, only the byte count). A segment VALIDATES when it meets no error; no distance reaches in front
//    of its own first output byte; no block in it has BFINAL set, unless it is the last segment; the decode stands at a block
//    boundary exactly at the segment's last byte with no bit left over; and, for the last segment, the BFINAL block ends inside it and
//    only zero bits up to the byte, and no further byte, follow. Segment 0 starts at the stream's true start; a segment that
//    validates ends where the next one starts; so when all validate, every assumed start was the true one and the concatenated output
//    is the serial decoder's. k_png_inflate_scan adds the counts up (an exclusive prefix sum: where each segment writes) and says
//    `parallel` when all validated and the counts sum to the expected size; k_png_inflate_write then decodes every segment again,
//    this time storing. Otherwise the frame falls back: k_png_inflate_serial, which is launched behind the write pass in any case,
//    returns at once when `parallel` is set and decodes the frame when it is not. Nothing waits for another wave: the passes are
//    launches in stream order. A segment is whatever the writer made one: nothing assumes 8 rows.
//
// 2. Adler-32 of the inflated stream (k_png_adler, k_png_check): with N bytes d[0..N), a = 1 + Σ d[i], b = N + Σ (N - i) d[i], both mod
//    65521 (png_kernels.hpp's per-row partial sums show the same decomposition). A thread sums 16-byte pieces: Σ d and Σ j d[j] of a
//    piece at i0 give its share of b as (N - i0) Σ d - Σ j d[j]. k_png_check compares with the staged trailer, looks at every row's
//    filter type (above 4: SFX_PNG_BAD_FILTER) and notes the first bad frame for sfx_video_status.
//
// 3. Unfilter (k_png_unfilter): Recon of filter types 0…4 with bpp = 3, zeros above row 0 and left of pixel 0, written into the RGB8
//    box with rows flipped (`bottom_up`). One workgroup; a wave works on a band of 64 consecutive rows, a lane per row, four pixels
//    (12 bytes) per step; lane l works one step behind lane l - 1 and receives that row's four pixels by a shuffle, so a band takes
//    ⌈W/4⌉ + 63 steps. Lane 0 reads the row above its band from the box, where the band above wrote it. The waves pipeline the bands:
//    wave w starts PNG_UNFILTER_LAG chunks of PNG_UNFILTER_CHUNK steps behind wave w - 1, with one __syncthreads per chunk — the
//    group lane 0 reads in chunk k was stored by the band above at its step 32k + 31 + 63 at the latest, inside its chunk k + 2. A
//    lane loads its row's next group of the inflated stream a step early. A frame with a bad status is not drawn: the box keeps its
//    content.
#pragma once

#include "jpeg_common.hpp"

namespace sf {

constexpr int PNG_FRAME_FIXED = sizeof(sfx_png_frame);
constexpr int PNG_WINDOW = 32768, PNG_FAST_BITS = 10, PNG_FLUSH = 256;
constexpr int PNG_UNFILTER_WAVES = 8, PNG_UNFILTER_CHUNK = 32, PNG_UNFILTER_LAG = 3;
constexpr uint32_t PNG_MAX_OUTPUT = 0x7fffffffu;                        // height x (1 + 3 width) at the most

struct PngSegmentRecord { uint32_t count, offset, valid, reserved; };
// control words of one frame's decode: [0] parallel (the segment path decoded it), [1] fell back; [2…7] the Adler sums as three 64-bit words
struct PngScratch {
    uint32_t* control;
    PngSegmentRecord* records; uint32_t capacity;                       // records there are
    uint8_t* filtered;                                                  // the inflated stream, expected + 64 bytes
};

struct PngCode {
    uint16_t fast[1 << PNG_FAST_BITS];
    uint16_t sorted[288];                                               // symbols by (length, symbol)
    uint16_t count[16];                                                 // codes per length
};
struct PngLds {
    uint8_t window[PNG_WINDOW];
    PngCode literal, distance;
    uint8_t lengths[320];
};

__constant__ uint8_t png_length_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct PngReader { const uint8_t* data; uint32_t pos, end; unsigned long long hold; int bits; };

__device__ __forceinline__ void png_fill(PngReader& r) {               // afterwards more than 32 bits are there, or all that are left
    if (r.bits <= 32 && r.pos < r.end) {
        uint32_t v = 0; uint32_t got = r.end - r.pos;
        if (got >= 4) { __builtin_memcpy(&v, r.data + r.pos, 4); got = 4; }
        else for (uint32_t k = 0; k < got; k++) v |= (uint32_t)r.data[r.pos + k] << (8*k);
        r.hold |= (unsigned long long)v << r.bits;
        r.bits += 8*(int)got; r.pos += got;
    }
}
// `count` ≤ 16 bits; -1 when fewer are left
__device__ __forceinline__ int png_take(PngReader& r, int count) {
    png_fill(r);
    if (r.bits < count) return -1;
    const int v = (int)(r.hold & ((1ull << count) - 1ull));
    r.hold >>= count; r.bits -= count;
    return v;
}

// The tables of one canonical code from `n` lengths in LDS; the whole wave calls it. false: over-subscribed.
__device__ __forceinline__ bool png_build(PngCode& code, const uint8_t* lengths, int n, int lane) {
    __syncthreads();                                                   // the lengths are written; nobody reads the old tables any more
    for (int k = lane; k < (1 << PNG_FAST_BITS); k += 64) code.fast[k] = 0;
    int count[16];
#pragma unroll
    for (int L = 0; L < 16; L++) count[L] = 0;
    for (int base = 0; base < n; base += 64) {
        const int mine = base + lane < n ? lengths[base + lane] : 0;
#pragma unroll
        for (int L = 1; L < 16; L++) count[L] += __popcll(__ballot(mine == L));
    }
    int left = 1;
#pragma unroll
    for (int L = 1; L < 16; L++) { left = (left << 1) - count[L]; if (left < 0) return false; }
    int next[16], place[16];
    next[0] = place[0] = 0; next[1] = 0; place[1] = 0;
#pragma unroll
    for (int L = 2; L < 16; L++) { next[L] = (next[L - 1] + count[L - 1]) << 1; place[L] = place[L - 1] + count[L - 1]; }
    if (lane < 16) code.count[lane] = 0;
    __syncthreads();
#pragma unroll
    for (int L = 1; L < 16; L++) if (lane == 0) code.count[L] = (uint16_t)count[L];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < n; base += 64) {
        const int symbol = base + lane, mine = symbol < n ? lengths[symbol] : 0;
#pragma unroll
        for (int L = 1; L < 16; L++) {
            const unsigned long long same = __ballot(mine == L);
            if (mine == L) {
                const int rank = __popcll(same & below);
                code.sorted[place[L] + rank] = (uint16_t)symbol;
                const uint32_t reversed = __brev((uint32_t)(next[L] + rank)) >> (32 - L);
                if (L <= PNG_FAST_BITS) for (uint32_t k = reversed; k < (1u << PNG_FAST_BITS); k += 1u << L) code.fast[k] = (uint16_t)((symbol << 4) | L);
                else code.fast[reversed & ((1u << PNG_FAST_BITS) - 1u)] = 0xffff;
            }
            next[L] += __popcll(same); place[L] += __popcll(same);
        }
    }
    __syncthreads();
    return true;
}

// The next symbol of `code`; -1: the bits match no code; -2: the bits ran out
__device__ __forceinline__ int png_symbol(PngReader& r, const PngCode& code) {
    png_fill(r);
    const uint32_t entry = code.fast[(uint32_t)r.hold & ((1u << PNG_FAST_BITS) - 1u)];
    if (entry != 0xffffu) {
        const int length = entry & 15;
        if (entry == 0u) return r.bits < PNG_FAST_BITS ? -2 : -1;
        if (length > r.bits) return -2;
        r.hold >>= length; r.bits -= length;
        return (int)(entry >> 4);
    }
    int value = 0, first = 0, index = 0;
    for (int length = 1; length < 16; length++) {
        if (r.bits < length) return -2;
        value |= (int)((r.hold >> (length - 1)) & 1ull);
        const int count = code.count[length];
        if (value - count < first) { r.hold >>= length; r.bits -= length; return code.sorted[index + (value - first)]; }
        index += count; first += count; first <<= 1; value <<= 1;
    }
    return -1;
}

// the ring's bytes [flushed, pos) → out, whole pieces of PNG_FLUSH bytes, and the rest too when `all`
__device__ __forceinline__ void png_flush(const PngLds& lds, uint8_t* out, uint32_t pos, uint32_t& flushed, int lane, bool all) {
    if (!out) { flushed = pos; return; }
    __syncthreads();
    while (pos - flushed >= (uint32_t)PNG_FLUSH) {                     // (flushed stays a multiple of 256: the ring is read as aligned words)
        const uint32_t at = flushed + 4u*lane;
        const uint32_t word = *(const uint32_t*)&lds.window[at & (PNG_WINDOW - 1)];
        __builtin_memcpy(out + at, &word, 4);
        flushed += PNG_FLUSH;
    }
    if (all) {
        for (uint32_t at = flushed + lane; at < pos; at += 64) out[at] = lds.window[at & (PNG_WINDOW - 1)];
        flushed = pos;
    }
}

struct PngInflated { uint32_t status, produced; bool valid; };
enum { PNG_RULE_SERIAL = 0, PNG_RULE_SEGMENT = 1, PNG_RULE_LAST_SEGMENT = 2 };

// Section 1 of the header comment. `out` null: nothing is stored (the count pass). `limit`: output bytes at the most.
__device__ __forceinline__ PngInflated png_inflate(PngLds& lds, const uint8_t* data, uint32_t begin, uint32_t end, uint8_t* out, uint32_t limit, int rule, int lane) {
    PngReader r{data, begin, end, 0ull, 0};
    uint32_t pos = 0, flushed = 0, status = 0;
    bool final_seen = false, fixed_built = false;
    for (;;) {
        if (rule != PNG_RULE_SERIAL && r.bits == 0 && r.pos == r.end) break;          // a block boundary at the segment's last byte
        const int header = png_take(r, 3);
        if (header < 0) { status |= SFX_PNG_OUT_OF_BITS; break; }
        const int type = header >> 1;
        if (type == 3) { status |= SFX_PNG_BAD_BLOCK; break; }
        if (type == 0) {
            const int pad = r.bits & 7;
            r.hold >>= pad; r.bits -= pad;
            const int length = png_take(r, 16), complement = png_take(r, 16);
            if (length < 0 || complement < 0) { status |= SFX_PNG_OUT_OF_BITS; break; }
            if ((length ^ complement) != 0xffff) { status |= SFX_PNG_BAD_STORED; break; }
            uint32_t from = r.pos - (uint32_t)(r.bits >> 3);                           // the whole bytes the reader holds go back
            r.hold = 0ull; r.bits = 0;
            if ((uint32_t)length > end - from) { status |= SFX_PNG_OUT_OF_BITS; break; }
            if ((uint32_t)length > limit - pos) { status |= SFX_PNG_BAD_SIZE; break; }
            uint32_t left = (uint32_t)length;
            while (left) {
                const uint32_t piece = left < 4096u ? left : 4096u;
                __syncthreads();
                for (uint32_t k = lane; k < piece; k += 64) lds.window[(pos + k) & (PNG_WINDOW - 1)] = data[from + k];
                pos += piece; from += piece; left -= piece;
                if (pos - flushed >= (uint32_t)PNG_FLUSH) png_flush(lds, out, pos, flushed, lane, false);
            }
            r.pos = from;
        } else {
            if (type == 1) {
                if (!fixed_built) {
                    __syncthreads();
                    for (int k = lane; k < 318; k += 64) lds.lengths[k] = (uint8_t)(k < 144 ? 8 : k < 256 ? 9 : k < 280 ? 7 : k < 288 ? 8 : 5);
                    png_build(lds.literal, lds.lengths, 288, lane);
                    png_build(lds.distance, lds.lengths + 288, 30, lane);
                    fixed_built = true;
                }
            } else {
                fixed_built = false;
                const int hlit = png_take(r, 5), hdist = png_take(r, 5), hclen = png_take(r, 4);
                if (hlit < 0 || hdist < 0 || hclen < 0) { status |= SFX_PNG_OUT_OF_BITS; break; }
                const int literals = hlit + 257, distances = hdist + 1, total = literals + distances;
                if (literals > 286 || distances > 30) { status |= SFX_PNG_BAD_LENGTHS; break; }
                __syncthreads();
                for (int k = 0; k < 19; k++) {
                    const int v = k < hclen + 4 ? png_take(r, 3) : 0;
                    if (v < 0) { status |= SFX_PNG_OUT_OF_BITS; break; }
                    lds.lengths[png_length_order[k]] = (uint8_t)v;
                }
                if (status) break;
                if (!png_build(lds.literal, lds.lengths, 19, lane)) { status |= SFX_PNG_BAD_LENGTHS; break; }
                int index = 0, previous = -1;
                while (index < total) {
                    const int symbol = png_symbol(r, lds.literal);
                    if (symbol < 0) { status |= symbol == -2 ? SFX_PNG_OUT_OF_BITS : SFX_PNG_BAD_CODE; break; }
                    if (symbol < 16) { lds.lengths[index++] = (uint8_t)symbol; previous = symbol; continue; }
                    int repeat, value = 0;
                    if (symbol == 16) {
                        if (previous < 0) { status |= SFX_PNG_BAD_LENGTHS; break; }
                        value = previous; repeat = png_take(r, 2); if (repeat >= 0) repeat += 3;
                    } else if (symbol == 17) { repeat = png_take(r, 3); if (repeat >= 0) repeat += 3; }
                    else { repeat = png_take(r, 7); if (repeat >= 0) repeat += 11; }
                    if (repeat < 0) { status |= SFX_PNG_OUT_OF_BITS; break; }
                    if (index + repeat > total) { status |= SFX_PNG_BAD_LENGTHS; break; }
                    for (int k = 0; k < repeat; k++) lds.lengths[index++] = (uint8_t)value;
                    previous = value;
                }
                if (status) break;
                __syncthreads();
                if (lds.lengths[256] == 0) { status |= SFX_PNG_BAD_LENGTHS; break; }
                // (the distance code first: building the literal code ends with a barrier, and the lengths are read by then)
                if (!png_build(lds.distance, lds.lengths + literals, distances, lane) || !png_build(lds.literal, lds.lengths, literals, lane)) { status |= SFX_PNG_BAD_LENGTHS; break; }
            }
            for (;;) {
                const int symbol = png_symbol(r, lds.literal);
                if (symbol < 0) { status |= symbol == -2 ? SFX_PNG_OUT_OF_BITS : SFX_PNG_BAD_CODE; break; }
                if (symbol < 256) {
                    if (pos >= limit) { status |= SFX_PNG_BAD_SIZE; break; }
                    lds.window[pos & (PNG_WINDOW - 1)] = (uint8_t)symbol;
                    pos++;
                } else if (symbol == 256) break;
                else {
                    if (symbol > 285) { status |= SFX_PNG_BAD_CODE; break; }
                    const int s = symbol - 257;
                    int length;
                    if (s < 8) length = 3 + s;
                    else if (s == 28) length = 258;
                    else {
                        const int extra = (s >> 2) - 1, more = png_take(r, extra);
                        if (more < 0) { status |= SFX_PNG_OUT_OF_BITS; break; }
                        length = 3 + ((4 + (s & 3)) << extra) + more;
                    }
                    const int d = png_symbol(r, lds.distance);
                    if (d < 0) { status |= d == -2 ? SFX_PNG_OUT_OF_BITS : SFX_PNG_BAD_CODE; break; }
                    if (d > 29) { status |= SFX_PNG_BAD_CODE; break; }
                    uint32_t distance;
                    if (d < 4) distance = 1u + d;
                    else {
                        const int extra = (d >> 1) - 1, more = png_take(r, extra);
                        if (more < 0) { status |= SFX_PNG_OUT_OF_BITS; break; }
                        distance = 1u + ((2u + (d & 1)) << extra) + (uint32_t)more;
                    }
                    if (distance > pos) { status |= SFX_PNG_BAD_DISTANCE; break; }
                    if ((uint32_t)length > limit - pos) { status |= SFX_PNG_BAD_SIZE; break; }
                    __syncthreads();
                    for (uint32_t k = lane; k < (uint32_t)length; k += 64) {
                        const uint32_t j = k < distance ? k : k % distance;
                        lds.window[(pos + k) & (PNG_WINDOW - 1)] = lds.window[(pos - distance + j) & (PNG_WINDOW - 1)];
                    }
                    pos += length;
                }
                if (pos - flushed >= (uint32_t)PNG_FLUSH) png_flush(lds, out, pos, flushed, lane, false);
            }
        }
        if (status) break;
        if (header & 1) { final_seen = true; break; }
    }
    PngInflated result{status, pos, false};
    if (status) return result;
    const int pad = r.bits & 7;
    const bool zero_pad = (r.hold & ((1ull << pad) - 1ull)) == 0ull;
    const bool at_end = (uint32_t)((r.bits - pad) >> 3) + (r.end - r.pos) == 0u;
    if (rule == PNG_RULE_SERIAL) {
        if (pos != limit) result.status |= SFX_PNG_BAD_SIZE;
        else if (!at_end) result.status |= SFX_PNG_BAD_ADLER;
    } else if (rule == PNG_RULE_LAST_SEGMENT) result.valid = final_seen && zero_pad && at_end;
    else result.valid = !final_seen && r.bits == 0 && r.pos == r.end;
    if (out && !result.status) png_flush(lds, out, pos, flushed, lane, true);
    return result;
}

// what the kernels refuse of a staged frame of `nbytes` bytes at the most (the host checked it; this keeps a damaged word from reaching an address)
__device__ __forceinline__ bool png_sane(const sfx_png_frame& f, int width, int height, uint32_t nbytes) {
    return f.magic == SFX_PNG_FRAME_MAGIC && f.width == (uint32_t)width && f.height == (uint32_t)height && f.segments >= 1u
           && f.payload_offset <= nbytes && f.payload_bytes <= nbytes - f.payload_offset && f.payload_offset >= (uint32_t)PNG_FRAME_FIXED
           && f.segments <= (f.payload_offset - (uint32_t)PNG_FRAME_FIXED)/4u;
}

__global__ void __launch_bounds__(64) k_png_inflate_count(const uint8_t* __restrict__ frame, PngScratch scratch, int width, int height, uint32_t nbytes, uint32_t expected) {
    __shared__ PngLds lds;
    const sfx_png_frame f = *(const sfx_png_frame*)frame;
    const uint32_t segment = blockIdx.x;
    const int lane = threadIdx.x;
    PngInflated result{0u, 0u, false};
    if (png_sane(f, width, height, nbytes) && segment < f.segments && segment < scratch.capacity) {
        const uint32_t* table = (const uint32_t*)(frame + PNG_FRAME_FIXED);
        const uint32_t begin = table[segment], end = segment + 1 < f.segments ? table[segment + 1] : f.payload_bytes;
        if (begin <= end && end <= f.payload_bytes)
            result = png_inflate(lds, frame + f.payload_offset, begin, end, nullptr, expected, segment + 1 == f.segments ? PNG_RULE_LAST_SEGMENT : PNG_RULE_SEGMENT, lane);
    }
    if (lane == 0 && segment < scratch.capacity) scratch.records[segment] = PngSegmentRecord{result.produced, 0u, result.valid ? 1u : 0u, 0u};
}

// `paths` (pinned host memory, or null): [0] frames the segment path decoded, [1] frames that fell back, counted here
__global__ void __launch_bounds__(64) k_png_inflate_scan(PngScratch scratch, uint32_t segments, uint32_t expected, volatile uint32_t* paths) {
    const int lane = threadIdx.x;
    unsigned long long carry = 0ull;
    bool all = segments <= scratch.capacity;
    for (uint32_t base = 0; all && base < segments; base += 64) {
        const uint32_t segment = base + lane;
        const uint32_t count = segment < segments ? scratch.records[segment].count : 0u;
        const uint32_t valid = segment < segments ? scratch.records[segment].valid : 1u;
        unsigned long long sum = count;                                  // (64 bits: 64 counts below 2^31 each)
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) { const unsigned long long other = __shfl_up(sum, step); if (lane >= step) sum += other; }
        if (segment < segments) scratch.records[segment].offset = (uint32_t)(carry + sum - count);    // (meaningful only while the sums stay within `expected`)
        carry += __shfl(sum, 63);
        all = __ballot(valid == 0u) == 0ull && carry <= (unsigned long long)expected;
    }
    if (lane == 0) {
        const uint32_t parallel = all && carry == (unsigned long long)expected ? 1u : 0u;
        scratch.control[0] = parallel; scratch.control[1] = parallel ^ 1u;
        if (paths) paths[parallel ^ 1u] = paths[parallel ^ 1u] + 1u;
    }
}

__global__ void __launch_bounds__(64) k_png_inflate_write(const uint8_t* __restrict__ frame, PngScratch scratch) {
    __shared__ PngLds lds;
    if (!scratch.control[0]) return;
    const sfx_png_frame f = *(const sfx_png_frame*)frame;               // (sane, and every segment in range: the count pass validated them all)
    const uint32_t segment = blockIdx.x;
    if (segment >= f.segments) return;
    const uint32_t* table = (const uint32_t*)(frame + PNG_FRAME_FIXED);
    const uint32_t begin = table[segment], end = segment + 1 < f.segments ? table[segment + 1] : f.payload_bytes;
    const PngSegmentRecord record = scratch.records[segment];
    png_inflate(lds, frame + f.payload_offset, begin, end, scratch.filtered + record.offset, record.count, segment + 1 == f.segments ? PNG_RULE_LAST_SEGMENT : PNG_RULE_SEGMENT, (int)threadIdx.x);
}

__global__ void __launch_bounds__(64) k_png_inflate_serial(const uint8_t* __restrict__ frame, PngScratch scratch, uint32_t* __restrict__ status, int width, int height, uint32_t nbytes, uint32_t expected) {
    __shared__ PngLds lds;
    if (scratch.control[0]) return;
    const sfx_png_frame f = *(const sfx_png_frame*)frame;
    uint32_t bits = SFX_PNG_BAD_DESCRIPTOR;
    if (png_sane(f, width, height, nbytes)) bits = png_inflate(lds, frame + f.payload_offset, 0u, f.payload_bytes, scratch.filtered, expected, PNG_RULE_SERIAL, (int)threadIdx.x).status;
    if (threadIdx.x == 0 && bits) atomicOr(status, bits);
}

// ---- 2. Adler-32 ------------------------------------------------------------------------------------------------------------------------
constexpr int PNG_ADLER_THREADS = 256, PNG_ADLER_PIECES = 4;            // a workgroup sums 256 x 4 pieces of 16 bytes

__global__ void __launch_bounds__(PNG_ADLER_THREADS) k_png_adler(PngScratch scratch, const uint32_t* __restrict__ status, uint32_t total) {
    if (*status) return;
    __shared__ unsigned long long sums[3];
    const int t = threadIdx.x;
    if (t < 3) sums[t] = 0ull;
    __syncthreads();
    unsigned long long plain = 0ull, weighted = 0ull, ramp = 0ull;
    for (int piece = 0; piece < PNG_ADLER_PIECES; piece++) {
        const unsigned long long at = ((unsigned long long)blockIdx.x*PNG_ADLER_PIECES + piece)*PNG_ADLER_THREADS*16ull + (unsigned long long)t*16ull;
        if (at >= total) break;
        uint32_t s = 0u, js = 0u;
        if (at + 16ull <= total) {
            const uint4 words = *(const uint4*)(scratch.filtered + at);
            const uint32_t w[4] = {words.x, words.y, words.z, words.w};
#pragma unroll
            for (int j = 0; j < 16; j++) { const uint32_t d = (w[j >> 2] >> (8*(j & 3))) & 255u; s += d; js += (uint32_t)j*d; }
        } else for (uint32_t j = 0; at + j < total; j++) { const uint32_t d = scratch.filtered[at + j]; s += d; js += j*d; }
        plain += s; ramp += js;
        weighted += (unsigned long long)((total - (uint32_t)at) % 65521u)*s;
    }
    atomicAdd(&sums[0], plain); atomicAdd(&sums[1], weighted); atomicAdd(&sums[2], ramp);
    __syncthreads();
    if (t < 3 && sums[t]) atomicAdd((unsigned long long*)(scratch.control + 2) + t, sums[t]);
}

__global__ void __launch_bounds__(256) k_png_check(const uint8_t* __restrict__ frame, PngScratch scratch, uint32_t* status, volatile uint32_t* first_bad, uint32_t serial,
                                                   int width, int height, uint32_t total) {
    const int t = threadIdx.x;
    uint32_t bits = *status;
    __syncthreads();
    if (!bits) {
        const size_t stride = 1 + 3*(size_t)width;
        int bad = 0;
        for (int row = t; row < height; row += 256) bad |= scratch.filtered[row*stride] > 4;
        if (__syncthreads_or(bad)) bits |= SFX_PNG_BAD_FILTER;
        const unsigned long long* sums = (const unsigned long long*)(scratch.control + 2);
        const uint32_t a = (uint32_t)((1ull + sums[0]) % 65521ull);
        const uint32_t b = (uint32_t)((total % 65521u + sums[1] % 65521ull + 65521ull - sums[2] % 65521ull) % 65521ull);
        if (((b << 16) | a) != ((const sfx_png_frame*)frame)->adler) bits |= SFX_PNG_BAD_ADLER;
        if (t == 0 && bits) *status = bits;
    }
    if (t == 0 && bits && first_bad && first_bad[0] == 0u) { first_bad[1] = serial; first_bad[0] = bits; }
}

// ---- 3. unfilter ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t png_byte(const uint32_t (&w)[3], int j) { return (w[j >> 2] >> (8*(j & 3))) & 255u; }

// 12 bytes at `p`, of which `live` are the row's (12: three word loads; the row's end otherwise: byte loads, zeros behind it)
__device__ __forceinline__ void png_load12(const uint8_t* p, int live, uint32_t (&w)[3]) {
    if (live >= 12) { __builtin_memcpy(&w[0], p, 4); __builtin_memcpy(&w[1], p + 4, 4); __builtin_memcpy(&w[2], p + 8, 4); return; }
    w[0] = w[1] = w[2] = 0u;
    for (int j = 0; j < live; j++) w[j >> 2] |= (uint32_t)p[j] << (8*(j & 3));
}

__global__ void __launch_bounds__(PNG_UNFILTER_WAVES*64) k_png_unfilter(const uint8_t* filtered, uint8_t* dst, const uint32_t* status, int width, int height, int bottom_up) {
    if (*status) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t stride = 1 + 3*(size_t)width, pitch = 3*(size_t)width;
    const int groups = (width + 3)/4, band_steps = groups + 63, chunks = (band_steps + PNG_UNFILTER_CHUNK - 1)/PNG_UNFILTER_CHUNK;
    const int bands = (height + 63)/64, rounds = (bands + PNG_UNFILTER_WAVES - 1)/PNG_UNFILTER_WAVES;
    const int period = chunks > PNG_UNFILTER_LAG*PNG_UNFILTER_WAVES ? chunks : PNG_UNFILTER_LAG*PNG_UNFILTER_WAVES;
    const long steps = (long)(rounds - 1)*period + PNG_UNFILTER_LAG*(PNG_UNFILTER_WAVES - 1) + chunks;
    // the band's state, a lane's row: the last group it wrote (a of the next one), the last pixel of the group above it (c of the next one)
    uint32_t mine[3] = {0u, 0u, 0u}, corner = 0u, type = 0u;
    uint32_t ahead[3] = {0u, 0u, 0u};                                  // the row's next group, loaded a step early (the inflated stream is read-only here)
    int row = -1, ahead_group = -1;
    const uint8_t *source = nullptr, *above = nullptr;
    uint8_t* target = nullptr;
    for (long step = 0; step < steps; step++) {
        const long since = step - (long)PNG_UNFILTER_LAG*wave;
        const int round = since >= 0 ? (int)(since/period) : -1, chunk = since >= 0 ? (int)(since - (long)round*period) : 0;
        const int band = round*PNG_UNFILTER_WAVES + wave;
        if (round >= 0 && round < rounds && band < bands && chunk < chunks) {
            if (chunk == 0) {
                row = band*64 + lane;
                mine[0] = mine[1] = mine[2] = 0u; corner = 0u; ahead_group = -1;
                const bool live = row < height;
                source = filtered + (live ? row*stride : 0) + 1;
                type = live ? filtered[row*stride] : 0u;
                target = dst + (live ? (size_t)(bottom_up ? height - 1 - row : row)*pitch : 0);
                above = lane == 0 && row > 0 ? dst + (size_t)(bottom_up ? height - row : row - 1)*pitch : nullptr;
            }
            for (int k = 0; k < PNG_UNFILTER_CHUNK; k++) {
                const int group = chunk*PNG_UNFILTER_CHUNK + k - lane;
                uint32_t up[3];
#pragma unroll
                for (int w = 0; w < 3; w++) up[w] = (uint32_t)__shfl_up((int)mine[w], 1);
                const bool work = row < height && group >= 0 && group < groups;
                if (!work) continue;
                const int live = min(12, 3*width - 12*group);
                if (lane == 0) { if (above) png_load12(above + 12*(size_t)group, live, up); else up[0] = up[1] = up[2] = 0u; }
                uint32_t in[3], out[3] = {0u, 0u, 0u};
                if (ahead_group == group) { in[0] = ahead[0]; in[1] = ahead[1]; in[2] = ahead[2]; }
                else png_load12(source + 12*(size_t)group, live, in);
                if (group + 1 < groups) { png_load12(source + 12*(size_t)(group + 1), min(12, 3*width - 12*(group + 1)), ahead); ahead_group = group + 1; }
                uint32_t recon[12];
#pragma unroll
                for (int j = 0; j < 12; j++) {
                    const int a = j < 3 ? (int)((mine[2] >> (8*(j + 1))) & 255u) : (int)recon[j - 3];
                    const int b = (int)png_byte(up, j);
                    const int c = j < 3 ? (int)((corner >> (8*j)) & 255u) : (int)png_byte(up, j - 3);
                    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2*c);
                    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                    const int predicted = type == 1u ? a : type == 2u ? b : type == 3u ? (a + b) >> 1 : type == 4u ? paeth : 0;
                    recon[j] = (png_byte(in, j) + (uint32_t)predicted) & 255u;
                    out[j >> 2] |= recon[j] << (8*(j & 3));
                }
                corner = up[2] >> 8;                                   // bytes 9, 10, 11 of the group above
                mine[0] = out[0]; mine[1] = out[1]; mine[2] = out[2];
                uint8_t* to = target + 12*(size_t)group;
                if (live >= 12) { __builtin_memcpy(to, &out[0], 4); __builtin_memcpy(to + 4, &out[1], 4); __builtin_memcpy(to + 8, &out[2], 4); }
                else for (int j = 0; j < live; j++) to[j] = (uint8_t)recon[j];
            }
        }
        __syncthreads();
    }
}

}  // namespace sf
