// jpeg_decode_kernels.hpp — baseline JPEG frames of a Motion-JPEG source on the device (capi_video.hip launches these):
// the inverse of jpeg_kernels.hpp, for streams other encoders wrote as well as this project's own.
//
// The decode is DEFINED here and restated in float64 by tests/jpeg_decode_ref.py:
//   * input: baseline sequential (SOF0), 8 bit, Huffman, ONE interleaved scan; three components read as JFIF YCbCr with luma sampling
//     2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4) and chroma 1x1, or one component (grey); 8-bit quantisation tables; the stream's own
//     Huffman tables (the host puts the standard's Annex K tables in their place when the stream has no DHT); any restart interval,
//     RSTn checked modulo 8. Everything else is refused by the host's header parser (mjpegsource.py) before a byte is staged;
//   * entropy decoding: the unit is the restart interval (the DC predictors are zero at its start, nothing crosses intervals). A
//     stream without restart markers is one interval: it decodes correctly, and serially;
//   * samples: coefficient times its quantiser (integers), 8 x 8 inverse DCT in f32 with the encoder's orthonormal basis
//     (dct[u][x] = C(u)/2 cos((2x + 1) u pi / 16)): along the rows first, tmp[v][x] = sum over u = 0…7 of F[v][u] dct[u][x], then down
//     the columns, s[y][x] = sum over v = 0…7 of tmp[v][x] dct[v][y], both as fma chains in that order; add 128, round half up
//     (floor(s + 128 + 0.5)), clip to 0…255;
//   * chroma upsampling: the centred triangle filter in integers, edges replicated at the component's OWN extent ceil(w h_c / h_max)
//     (rows alike), not at the MCU padding:
//       2x1: even output (3 c[j] + c[j-1] + 1) >> 2, odd output (3 c[j] + c[j+1] + 2) >> 2;
//       2x2: column sums s = 3 near_row + far_row (the far row is the one above for an even output row, below for an odd one),
//            even output (3 s[j] + s[j-1] + 8) >> 4, odd output (3 s[j] + s[j+1] + 7) >> 4;
//   * colour, full range, 16-bit fixed point, arithmetic shifts, Cb' = Cb - 128, Cr' = Cr - 128, each clipped to 0…255:
//       R = Y + (( 91881 Cr' + 32768) >> 16)
//       G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16)
//       B = Y + ((116130 Cb' + 32768) >> 16)                         grey: R = G = B = Y;
//   * output: the module's RGB8 texture, rows bottom-up, exactly as k_video_frame writes it.
//
// A staged frame (what the host's reader puts into a slot) is `sfx_jpeg_frame` (include/shaderflow_hip.h: the six words, the components'
// table selectors, four quantisation tables in zigzag order, four Huffman tables as BITS and HUFFVAL), one word per restart interval
// behind it (the host's reader finds the FF D0…D7 pairs with numpy: DESIGN.md §7c says why), then, 16-byte aligned, the scan.
// The host validates the words when a frame is submitted (capi_video.hip); the kernels check them again and clamp what they index with.
//
// Three kernels on the render stream:
//   k_jpeg_decode_entropy  a lane per restart interval (a wave serves 64 of them), one launch per staged frame: the Huffman lookups are built
//                          in LDS from the frame's own tables, the int16 coefficients leave in zigzag order, MCU by MCU (the encoder's
//                          layout). Every read is bounded by the interval's end and every loop by 64 terms and the interval's MCU count.
//                          A code that matches nothing, a run past 63, a missing or wrong RSTn and bits running out set bits of the
//                          frame's status word — never a fault, never a write outside the frame's scratch;
//   k_jpeg_decode_planes   dequantisation and the inverse DCT through LDS, four blocks per workgroup → the components' 8-bit planes;
//   k_jpeg_decode_pixels   upsampling, colour, row flip, RGB8 stores: a lane per run of 16 pixels, 16-byte aligned stores when the row
//                          pitch allows, heads and tails as k_video_frame's planar path has them.
// The pixel stage is two launches, not one: the triangle filter reads a ring of samples of the eight neighbouring chroma blocks, and a
// fused kernel would transform those blocks again per MCU (3.7 times the arithmetic at 4:2:0) to save 1.5 bytes per pixel written and
// read once (counted, not measured: DESIGN.md §7c).
#pragma once

#include "jpeg_common.hpp"

namespace sf {

constexpr int JPEG_FRAME_FIXED = sizeof(sfx_jpeg_frame);               // the interval table starts here

struct JpegDecodeGeometry {
    int width, height;
    int components;                 // 3 (YCbCr) or 1 (grey)
    int hs, vs;                     // luma sampling factors: 2x2, 2x1 or 1x1 (chroma, and grey, 1x1)
    int mcus_x, mcus_y, blocks;     // MCUs per row, MCU rows, blocks per MCU (hs*vs + 2, or 1)
    int capacity;                   // bytes of a staged frame at the most
};

inline size_t jpeg_decode_coefficients(const JpegDecodeGeometry& g) { return (size_t)g.mcus_x*g.mcus_y*g.blocks*64; }
__host__ __device__ inline size_t jpeg_plane_offset(const JpegDecodeGeometry& g, int component) {
    const size_t luma = (size_t)g.mcus_x*g.hs*8*g.mcus_y*g.vs*8, chroma = (size_t)g.mcus_x*8*g.mcus_y*8;
    return component == 0 ? 0 : luma + (component - 1)*chroma;
}
inline size_t jpeg_plane_bytes(const JpegDecodeGeometry& g) { return jpeg_plane_offset(g, g.components); }

// ---- 1. Huffman decoding, a lane per restart interval ------------------------------------------------------------------------------
// The bit reader keeps up to 64 bits, right-aligned. Past the interval's end, or at a marker inside it, it feeds zero bits and counts
// them (`fake`): they sit below the real ones, so real bits have run out exactly when fewer than `fake` bits are left.
struct JpegBitReader {
    const uint8_t* p; const uint8_t* end;
    unsigned long long acc; int n, fake;
};

__device__ __forceinline__ void jpeg_fill(JpegBitReader& r) {         // afterwards at least 57 bits are there
    while (r.n <= 56) {
        uint32_t byte = 0; bool real = false;
        if (r.p < r.end) {
            byte = *r.p;
            if (byte != 0xffu) { r.p++; real = true; }
            else if (r.p + 1 < r.end && r.p[1] == 0) { r.p += 2; real = true; }      // a stuffed FF
            else { r.end = r.p; byte = 0; }                              // a marker, or an FF the interval ends in: the data ends here
        }
        if (!real) r.fake += 8;
        r.acc = (r.acc << 8) | byte; r.n += 8;
    }
}
__device__ __forceinline__ int jpeg_take(JpegBitReader& r, int count) { // count ≤ 16 ≤ r.n
    r.n -= count;
    return (int)((r.acc >> r.n) & ((1ull << count) - 1ull));
}
__device__ __forceinline__ int jpeg_extend(int value, int size) { return (size == 0 || value >= (1 << (size - 1))) ? value : value - (1 << size) + 1; }

__global__ void __launch_bounds__(64) k_jpeg_decode_entropy(const uint8_t* __restrict__ frame, int16_t* __restrict__ coefficients, uint32_t* __restrict__ status,
                                                            JpegDecodeGeometry g) {
    __shared__ uint16_t lookup[4][256];                                 // the next 8 bits → (length << 8) | symbol; 0: a longer code, or none
    __shared__ int maxcode[4][17], valoff[4][17];                       // Annex F.2.2.3: the largest code of each length (-1: none), VALPTR - MINCODE
    __shared__ uint8_t values[4][256];
    const int lane = threadIdx.x;
    const sfx_jpeg_frame& f = *reinterpret_cast<const sfx_jpeg_frame*>(frame);
    const uint32_t scan_bytes = f.scan_bytes, restart = f.restart, intervals = f.intervals, scan_offset = f.scan_offset;
    const unsigned long long total = (unsigned long long)g.mcus_x*g.mcus_y;
    const bool sane = jpeg_descriptor_fault(f, g.mcus_x, g.mcus_y, (unsigned long long)g.capacity) == 0;
    if (!sane) {                                                        // (uniform: the whole workgroup leaves)
        if (blockIdx.x == 0 && lane == 0) atomicOr(status, SFX_JPEG_BAD_DESCRIPTOR);
        return;
    }
    for (int k = lane; k < 4*256; k += 64) values[k >> 8][k & 255] = f.huffman[k >> 8].values[k & 255];
    if (lane < 4) {
        const uint8_t* bits = f.huffman[lane].bits;
        int code = 0, first = 0;
        for (int length = 1; length <= 16; length++) {
            const int count = bits[length - 1];
            valoff[lane][length] = first - code;
            maxcode[lane][length] = count ? code + count - 1 : -1;
            first += count; code = (code + count) << 1;
        }
    }
    __syncthreads();
    for (int k = lane; k < 4*256; k += 64) {
        const int table = k >> 8, peek = k & 255;
        uint32_t entry = 0;
        for (int length = 1; length <= 8; length++) {
            const int code = peek >> (8 - length);
            if (code <= maxcode[table][length]) {
                const int at = valoff[table][length] + code;
                if (at >= 0 && at < 256) entry = ((uint32_t)length << 8) | values[table][at];
                break;
            }
        }
        lookup[table][peek] = (uint16_t)entry;
    }
    __syncthreads();

    const uint32_t interval = blockIdx.x*64u + (uint32_t)lane;
    if (interval >= intervals) return;
    const uint32_t* offsets = reinterpret_cast<const uint32_t*>(frame + JPEG_FRAME_FIXED);
    const uint8_t* scan = frame + scan_offset;
    const unsigned long long begin = offsets[interval], finish = interval + 1u < intervals ? (unsigned long long)offsets[interval + 1u] : (unsigned long long)scan_bytes + 2ull;
    uint32_t flags = 0;
    if (begin > scan_bytes || finish < begin + 2ull || finish > (unsigned long long)scan_bytes + 2ull) flags = SFX_JPEG_BAD_RESTART;      // this interval's marker, or the next one's, is missing
    else if (interval > 0u && (begin < 2ull || scan[begin - 2] != 0xffu || scan[begin - 1] != 0xd0u + ((interval - 1u) & 7u))) flags = SFX_JPEG_BAD_RESTART;
    if (flags) { atomicOr(status, flags); return; }

    JpegBitReader reader{scan + begin, scan + (finish - 2ull), 0ull, 0, 0};
    const int luma_blocks = g.components == 1 ? 1 : g.hs*g.vs;
    const unsigned long long first_mcu = (unsigned long long)interval*restart;
    const int mcus = (int)(total - first_mcu < restart ? total - first_mcu : restart);
    int16_t* out = coefficients + (size_t)first_mcu*g.blocks*64;
    int predictor0 = 0, predictor1 = 0, predictor2 = 0;

    // one Huffman symbol of table `table` (0, 1: DC; 2, 3: AC); -1 when no code matches
    auto symbol = [&](int table) -> int {
        jpeg_fill(reader);
        const int peek = (int)((reader.acc >> (reader.n - 16)) & 0xffffull);
        const uint32_t entry = lookup[table][peek >> 8];
        if (entry) { reader.n -= (int)(entry >> 8); return (int)(entry & 255u); }
        for (int length = 1; length <= 16; length++) {
            const int code = peek >> (16 - length);
            if (code <= maxcode[table][length]) {
                const int at = valoff[table][length] + code;
                if (at < 0 || at >= 256) return -1;
                reader.n -= length;
                return values[table][at];
            }
        }
        return -1;
    };

    for (int m = 0; m < mcus && !flags; m++) {
        for (int b = 0; b < g.blocks && !flags; b++, out += 64) {
            const int component = b < luma_blocks ? 0 : b - luma_blocks + 1;
            const int dc_table = f.td[component] & 1, ac_table = 2 + (f.ta[component] & 1);
            for (int k = 0; k < 8; k++) reinterpret_cast<uint4*>(out)[k] = make_uint4(0u, 0u, 0u, 0u);
            int size = symbol(dc_table);
            if (size < 0 || size > 15) { flags |= SFX_JPEG_BAD_CODE; break; }
            const int difference = jpeg_extend(jpeg_take(reader, size), size);
            int& predictor = component == 0 ? predictor0 : (component == 1 ? predictor1 : predictor2);
            predictor += difference;
            out[0] = (int16_t)predictor;
            int k = 1;
            for (int term = 0; term < 64 && k < 64; term++) {
                const int code = symbol(ac_table);
                if (code < 0) { flags |= SFX_JPEG_BAD_CODE; break; }
                const int run = code >> 4;
                size = code & 15;
                if (size == 0) {
                    if (run != 15) break;                               // EOB
                    k += 16;
                    if (k > 64) { flags |= SFX_JPEG_BAD_RUN; break; }
                    continue;
                }
                k += run;
                if (k > 63) { flags |= SFX_JPEG_BAD_RUN; break; }
                out[k++] = (int16_t)jpeg_extend(jpeg_take(reader, size), size);
            }
            if (reader.n < reader.fake) flags |= SFX_JPEG_OUT_OF_BITS;
        }
    }
    if (flags) atomicOr(status, flags);
}

// ---- 2. dequantisation and the inverse DCT → the components' planes --------------------------------------------------------------------
// 256 threads = four 8 x 8 blocks, a thread per term in both passes. The planes are padded to whole MCUs: luma mcus_x*hs*8 wide,
// chroma mcus_x*8. A frame whose status is bad is left alone (the texture keeps what it showed); the first such frame since the last
// question is noted in `first_bad` = {status, serial} (pinned host memory) for sfx_video_status.
__global__ void __launch_bounds__(256) k_jpeg_decode_planes(const sfx_jpeg_frame* __restrict__ frame, const int16_t* __restrict__ coefficients, uint8_t* __restrict__ planes,
                                                            const float* __restrict__ basis, const uint32_t* __restrict__ status, volatile uint32_t* first_bad, uint32_t serial,
                                                            JpegDecodeGeometry g) {
    __shared__ float dct[64];
    __shared__ float terms[4][64], rows[4][64];
    __shared__ __attribute__((aligned(8))) uint8_t samples[4][64];
    const int t = threadIdx.x, q = t >> 6, k = t & 63;
    const uint32_t bad = *status;
    if (bad) {
        if (first_bad && blockIdx.x == 0 && t == 0 && first_bad[0] == 0u) { first_bad[1] = serial; first_bad[0] = bad; }
        return;
    }
    const size_t total = (size_t)g.mcus_x*g.mcus_y*g.blocks, block = (size_t)blockIdx.x*4 + q;
    const bool live = block < total;
    const int luma_blocks = g.components == 1 ? 1 : g.hs*g.vs;
    const size_t mcu = block/g.blocks;
    const int b = (int)(block - mcu*g.blocks), component = b < luma_blocks ? 0 : b - luma_blocks + 1;
    if (t < 64) dct[t] = basis[t];
    int value = 0;
    if (live) value = (int)coefficients[block*64 + k]*(int)frame->quant[frame->tq[component] & 3][k];
    terms[q][JPEG_ZIGZAG.natural_of[k]] = (float)value;
    __syncthreads();
    const int hi = k >> 3, lo = k & 7;
    float acc = 0.0f;
#pragma unroll
    for (int u = 0; u < 8; u++) acc = fmaf(terms[q][hi*8 + u], dct[u*8 + lo], acc);       // row v = hi of the block's terms → sample column x = lo
    rows[q][k] = acc;
    __syncthreads();
    acc = 0.0f;
#pragma unroll
    for (int v = 0; v < 8; v++) acc = fmaf(rows[q][v*8 + lo], dct[v*8 + hi], acc);        // column x = lo → sample row y = hi
    const float rounded = floorf(acc + 128.0f + 0.5f);
    samples[q][k] = (uint8_t)(rounded < 0.0f ? 0.0f : (rounded > 255.0f ? 255.0f : rounded));
    __syncthreads();
    if (t < 32) {                                                       // a sample row of 8 bytes per thread
        const int group = t >> 3, row = t & 7;
        const size_t mine = (size_t)blockIdx.x*4 + group;
        if (mine < total) {
            const size_t at = mine/g.blocks;
            const int mb = (int)(mine - at*g.blocks), mc = mb < luma_blocks ? 0 : mb - luma_blocks + 1;
            const int mx = (int)(at % g.mcus_x), my = (int)(at/g.mcus_x);
            const int bx = mc == 0 && g.components == 3 ? mx*g.hs + mb % g.hs : mx, by = mc == 0 && g.components == 3 ? my*g.vs + mb/g.hs : my;
            const size_t pitch = (size_t)g.mcus_x*8*(mc == 0 && g.components == 3 ? g.hs : 1);
            *reinterpret_cast<uint2*>(planes + jpeg_plane_offset(g, mc) + ((size_t)by*8 + row)*pitch + (size_t)bx*8) = *reinterpret_cast<const uint2*>(&samples[group][row*8]);
        }
    }
}

// ---- 3. upsampling, colour, row flip → RGB8 -------------------------------------------------------------------------------------------
constexpr int JPEG_RUN = 16;                                        // pixels per lane

__device__ __forceinline__ int jpeg_clamp(int v, int last) { return v < 0 ? 0 : (v > last ? last : v); }       // into 0…last
__device__ __forceinline__ uint32_t jpeg_clip8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// the upsampled chroma of the 16 pixels from x0 on row y (x0 a multiple of 16): the triangle filter of the header's definition
__device__ __forceinline__ void jpeg_chroma_run(const uint8_t* __restrict__ plane, int pitch, int cw, int ch, int hs, int vs, int x0, int y, int (&out)[JPEG_RUN]) {
    if (hs == 1) {
        const uint8_t* row = plane + (size_t)y*pitch;
#pragma unroll
        for (int i = 0; i < JPEG_RUN; i++) out[i] = row[jpeg_clamp(x0 + i, cw - 1)];
        return;
    }
    const int near = y/vs, far = jpeg_clamp(near + ((y & 1) ? 1 : -1), ch - 1);
    const uint8_t* a = plane + (size_t)near*pitch;
    const uint8_t* b = plane + (size_t)far*pitch;
    int s[JPEG_RUN/2 + 2];
#pragma unroll
    for (int i = 0; i < JPEG_RUN/2 + 2; i++) {
        const int j = jpeg_clamp(x0/2 - 1 + i, cw - 1);
        s[i] = vs == 2 ? 3*(int)a[j] + (int)b[j] : (int)a[j];
    }
#pragma unroll
    for (int i = 0; i < JPEG_RUN; i++) {
        const int sum = 3*s[i/2 + 1] + ((i & 1) ? s[i/2 + 2] : s[i/2]);
        out[i] = vs == 2 ? (sum + ((i & 1) ? 7 : 8)) >> 4 : (sum + ((i & 1) ? 2 : 1)) >> 2;
    }
}

__global__ void __launch_bounds__(256) k_jpeg_decode_pixels(const uint8_t* __restrict__ planes, uint8_t* __restrict__ dst, const uint32_t* __restrict__ status,
                                                            JpegDecodeGeometry g, int bottom_up) {
    if (*status) return;
    const int w = g.width, h = g.height, runs = (w + JPEG_RUN - 1)/JPEG_RUN;
    const long index = (long)blockIdx.x*256 + threadIdx.x;
    if (index >= (long)runs*h) return;
    const int y = (int)(index/runs), x0 = ((int)(index - (long)y*runs))*JPEG_RUN;
    const int n = (w - x0) < JPEG_RUN ? (w - x0) : JPEG_RUN;
    const bool colour = g.components == 3;
    const int luma_pitch = g.mcus_x*8*(colour ? g.hs : 1);
    const uint8_t* lp = planes + (size_t)y*luma_pitch + x0;
    int luma[JPEG_RUN], cb[JPEG_RUN], cr[JPEG_RUN];
    if (x0 + JPEG_RUN <= luma_pitch) {
        uint32_t l[4]; __builtin_memcpy(l, lp, 16);
#pragma unroll
        for (int i = 0; i < JPEG_RUN; i++) luma[i] = (int)((l[i >> 2] >> (8*(i & 3))) & 255u);
    } else {
#pragma unroll
        for (int i = 0; i < JPEG_RUN; i++) luma[i] = i < n ? (int)lp[i] : 0;
    }
    if (colour) {
        const int cw = (w + g.hs - 1)/g.hs, ch = (h + g.vs - 1)/g.vs, pitch = g.mcus_x*8;
        jpeg_chroma_run(planes + jpeg_plane_offset(g, 1), pitch, cw, ch, g.hs, g.vs, x0, y, cb);
        jpeg_chroma_run(planes + jpeg_plane_offset(g, 2), pitch, cw, ch, g.hs, g.vs, x0, y, cr);
    }
    uint32_t out[12];
#pragma unroll
    for (int k = 0; k < 12; k++) out[k] = 0u;
#pragma unroll
    for (int i = 0; i < JPEG_RUN; i++) {
        uint32_t rgb[3];
        if (colour) {
            const int d = cb[i] - 128, e = cr[i] - 128;
            rgb[0] = jpeg_clip8(luma[i] + ((91881*e + 32768) >> 16));
            rgb[1] = jpeg_clip8(luma[i] + ((-22554*d - 46802*e + 32768) >> 16));
            rgb[2] = jpeg_clip8(luma[i] + ((116130*d + 32768) >> 16));
        } else rgb[0] = rgb[1] = rgb[2] = (uint32_t)luma[i];
#pragma unroll
        for (int k = 0; k < 3; k++) { const int at = 3*i + k; out[at >> 2] |= rgb[k] << (8*(at & 3)); }
    }
    uint8_t* o = dst + ((size_t)(bottom_up ? h - 1 - y : y)*w + x0)*3;
    if (n == JPEG_RUN && w % JPEG_RUN == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {   // every row starts on a 16-byte boundary: three aligned stores
#pragma unroll
        for (int k = 0; k < 3; k++) reinterpret_cast<uint4*>(o)[k] = make_uint4(out[4*k], out[4*k + 1], out[4*k + 2], out[4*k + 3]);
    } else if (n == JPEG_RUN) {
        __builtin_memcpy(o, out, 48);
    } else {
#pragma unroll
        for (int i = 0; i < 3*JPEG_RUN; i++) if (i < 3*n) o[i] = (uint8_t)(out[i >> 2] >> (8*(i & 3)));
    }
}
inline long jpeg_pixel_lanes(int w, int h) { return (long)((w + JPEG_RUN - 1)/JPEG_RUN)*h; }

}  // namespace sf
