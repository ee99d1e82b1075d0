// jpeg_common.hpp — what the Motion-JPEG encoder (jpeg_kernels.hpp, capi_jpeg.hip) and decoder (jpeg_decode_kernels.hpp, capi_video_jpeg.hip)
// share, each stated once: the zigzag order, the DCT basis, the standard's Annex K tables, and the test a staged frame's descriptor
// (include/shaderflow_hip.h: sfx_jpeg_frame) must pass before a kernel indexes anything with it.
#pragma once

#include "../../include/shaderflow_hip.h"
#include <hip/hip_runtime.h>
#include <cmath>

namespace sf {

// ---- the zigzag order ------------------------------------------------------------------------------------------------------------------
struct JpegZigzag {
    uint8_t natural_of[64];         // zigzag position → natural (row-major) index
    uint8_t zigzag_of[64];          // natural index → zigzag position
};
constexpr JpegZigzag jpeg_zigzag_walk() {                           // anti-diagonals, alternating direction
    JpegZigzag z{};
    for (int sum = 0, n = 0; sum < 15; sum++)
        for (int k = 0; k <= sum; k++) {
            const int row = (sum & 1) ? k : sum - k, col = sum - row;
            if (row < 8 && col < 8) { z.natural_of[n] = (uint8_t)(row*8 + col); z.zigzag_of[row*8 + col] = (uint8_t)n; n++; }
        }
    return z;
}
constexpr JpegZigzag JPEG_ZIGZAG = jpeg_zigzag_walk();              // (a constant on the host and, promoted by the compiler, on the device)
constexpr bool jpeg_zigzag_inverse(const JpegZigzag& z) {
    for (int k = 0; k < 64; k++)
        if (z.zigzag_of[z.natural_of[k]] != k || z.natural_of[z.zigzag_of[k]] != k) return false;
    return true;
}
static_assert(jpeg_zigzag_inverse(JPEG_ZIGZAG), "natural_of and zigzag_of are each other's inverse");
static_assert(JPEG_ZIGZAG.natural_of[0] == 0 && JPEG_ZIGZAG.natural_of[1] == 1 && JPEG_ZIGZAG.natural_of[2] == 8 && JPEG_ZIGZAG.natural_of[3] == 16
              && JPEG_ZIGZAG.natural_of[4] == 9 && JPEG_ZIGZAG.natural_of[5] == 2, "the standard's Figure A.6 begins 0, 1, 8, 16, 9, 2");

// ---- the DCT basis: out[u][x] = C(u)/2 cos((2x + 1) u pi / 16), computed in double and rounded once. Both handles upload it. ------------
inline void jpeg_dct_basis(float out[64]) {
    for (int u = 0; u < 8; u++)
        for (int x = 0; x < 8; x++) out[u*8 + x] = (float)((u == 0 ? std::sqrt(0.125) : 0.5)*std::cos((2*x + 1)*u*M_PI/16.0));
}

// ---- the standard's Annex K tables: quantisation in natural order, Huffman as BITS / HUFFVAL -------------------------------------------
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
static const uint8_t DC_LUMINANCE_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t DC_LUMINANCE_VALUES[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t DC_CHROMINANCE_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t DC_CHROMINANCE_VALUES[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t AC_LUMINANCE_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
static const uint8_t AC_LUMINANCE_VALUES[162] = {
    1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177,
    193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55,
    56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106,
    115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
    164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
    212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250,
};
static const uint8_t AC_CHROMINANCE_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
static const uint8_t AC_CHROMINANCE_VALUES[162] = {
    0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193,
    9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54,
    55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105,
    106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
    162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
    210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250,
};

// ---- a staged frame's descriptor -------------------------------------------------------------------------------------------------------
__host__ __device__ inline unsigned long long jpeg_interval_table_bytes(unsigned long long intervals) { return (intervals*4ull + 15ull) & ~15ull; }

// Whether the six words of a staged frame of a `mcus_x` x `mcus_y` picture fit each other and `limit` bytes (the host: the frame's
// length; the entropy kernel: the slots' capacity): the magic, a restart interval of at least one MCU, the interval count that follows
// from it, the scan right behind the interval table and inside the limit. 0: they do; else which test failed first (1: magic, 2: intervals, 3: scan).
__host__ __device__ inline int jpeg_descriptor_fault(const sfx_jpeg_frame& f, int mcus_x, int mcus_y, unsigned long long limit) {
    const unsigned long long total = (unsigned long long)mcus_x*mcus_y, restart = f.restart, intervals = f.intervals, scan_offset = f.scan_offset;
    if (f.magic != SFX_JPEG_FRAME_MAGIC) return 1;
    if (restart < 1ull || intervals != (total + restart - 1ull)/restart) return 2;
    if (scan_offset != (unsigned long long)sizeof(sfx_jpeg_frame) + jpeg_interval_table_bytes(intervals) || scan_offset + f.scan_bytes > limit) return 3;
    return 0;
}

}  // namespace sf
