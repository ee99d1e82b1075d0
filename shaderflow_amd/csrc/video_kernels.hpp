// video_kernels.hpp — k_video_frame: one staged source frame of a ShaderVideo (device memory, top row first) → the module's RGB8 video
// texture (3 bytes per texel, pitch width*3, rows bottom-up). What ShaderVideo.update() does on the host for every source frame
// (reference: shaderflow/video.py:57-66 — next frame, flipped to GL order, written into the texture) as one launch on the render stream.
//
// Two source layouts (include/shaderflow_hip.h):
//   SFX_VIDEO_RGB24  height x width x 3 bytes. The rows are copied in reverse order (np.flip(frame, axis=0)); any extents.
//   SFX_VIDEO_I420   planar 4:2:0: Y (height rows of width), U, V (height/2 rows of width/2), even extents. Rows flipped, every pixel
//                    converted with BT.601 limited range in integer arithmetic, chroma replicated over its 2 x 2 block (no interpolation):
//                      C = Y - 16, D = U - 128, E = V - 128
//                      R = clip8((298 C + 409 E + 128) >> 8)
//                      G = clip8((298 C - 100 D - 208 E + 128) >> 8)
//                      B = clip8((298 C + 516 D + 128) >> 8)            (arithmetic shifts of signed 32-bit values)
//                    The counterpart of k_rgb_to_yuv420 (capi_readout.hip) and, like it, DEFINED here: unpinned against swscale (no ffmpeg
//                    binary exists in this environment to pin swscale's against). tests/test_gpu_video.py restates it in numpy.
//
// Memory-bound, no LDS, no atomics, plain vector stores. Consecutive lanes take consecutive 16-byte pieces (rgb24) or consecutive runs
// of 16 pixels on two rows (I420: 2 x 16 B of Y, 8 B of U and of V in, 2 x 48 B out, so a chroma sample is loaded once). A packed RGB8
// row is 16-byte aligned from row to row only when width % 16 == 0: otherwise the rgb24 path stores the aligned pieces of the
// DESTINATION row whole and the row's head and tail byte by byte, and the I420 path stores its whole runs through unaligned vector
// accesses and the row's last, shorter run byte by byte.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace sf {

constexpr int VIDEO_THREADS = 256;
constexpr int VIDEO_RUN = 16;                                         // pixels per lane and row of the I420 path

__device__ __forceinline__ uint4 video_load16(const uint8_t* p) {
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const uint4*>(p);
    uint4 v; __builtin_memcpy(&v, p, 16); return v;                    // (an unaligned vector load where the target allows it)
}

// rgb24: piece 0 of a destination row is its head (the bytes in front of the first 16-byte boundary), the last piece its tail
__device__ __forceinline__ void video_frame_rgb24(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h) {
    const long row_bytes = 3L*w;
    const int per_row = (int)(row_bytes/16) + 2;
    const long index = (long)blockIdx.x*VIDEO_THREADS + threadIdx.x;
    if (index >= (long)per_row*h) return;
    const int j = (int)(index/per_row), piece = (int)(index - (long)j*per_row);
    const long begin = j*row_bytes, end = begin + row_bytes;           // the destination row's bytes
    const long from = (long)(h - 1 - j)*row_bytes - begin;             // source byte = destination byte + from
    long lo = ((begin + 15) & ~15L) + 16L*(piece - 1), hi = lo + 16;
    if (lo >= begin && hi <= end) {
        *reinterpret_cast<uint4*>(dst + lo) = video_load16(src + lo + from);
        return;
    }
    lo = lo > begin ? lo : begin; hi = hi < end ? hi : end;
    for (long b = lo; b < hi; b++) dst[b] = src[b + from];
}

__device__ __forceinline__ uint32_t video_clip8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// 16 pixels of one row: y[4] = their luma bytes, u[2] / v[2] = the 8 chroma bytes they share pairwise → 48 packed RGB bytes in out[12]
__device__ __forceinline__ void video_convert_run(const uint32_t (&y)[4], const uint32_t (&u)[2], const uint32_t (&v)[2], uint32_t (&out)[12]) {
#pragma unroll
    for (int k = 0; k < 12; k++) out[k] = 0u;
#pragma unroll
    for (int i = 0; i < VIDEO_RUN; i++) {
        const int c = 298*((int)((y[i >> 2] >> (8*(i & 3))) & 255u) - 16);
        const int d = (int)((u[i >> 3] >> (8*((i >> 1) & 3))) & 255u) - 128, e = (int)((v[i >> 3] >> (8*((i >> 1) & 3))) & 255u) - 128;
        const uint32_t rgb[3] = {video_clip8((c + 409*e + 128) >> 8), video_clip8((c - 100*d - 208*e + 128) >> 8), video_clip8((c + 516*d + 128) >> 8)};
#pragma unroll
        for (int k = 0; k < 3; k++) { const int b = 3*i + k; out[b >> 2] |= rgb[k] << (8*(b & 3)); }
    }
}

// I420: one lane = one run of 16 pixels on source rows 2p and 2p + 1 (destination rows h - 1 - 2p and h - 2 - 2p)
__device__ __forceinline__ void video_frame_i420(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h) {
    const int runs = (w + VIDEO_RUN - 1)/VIDEO_RUN;
    const long index = (long)blockIdx.x*VIDEO_THREADS + threadIdx.x;
    if (index >= (long)runs*(h/2)) return;
    const int p = (int)(index/runs), x0 = ((int)(index - (long)p*runs))*VIDEO_RUN;
    const int n = (w - x0) < VIDEO_RUN ? (w - x0) : VIDEO_RUN;          // pixels of this run (even: w is)
    const uint8_t* ya = src + (long)(2*p)*w + x0;
    const uint8_t* yb = ya + w;
    const uint8_t* up = src + (long)w*h + (long)p*(w/2) + x0/2;
    const uint8_t* vp = up + (long)(w/2)*(h/2);
    uint8_t* oa = dst + ((long)(h - 1 - 2*p)*w + x0)*3;
    uint8_t* ob = oa - 3L*w;
    uint32_t a[4] = {0u, 0u, 0u, 0u}, b[4] = {0u, 0u, 0u, 0u}, u[2] = {0u, 0u}, v[2] = {0u, 0u};
    if (n == VIDEO_RUN) {
        const uint4 la = video_load16(ya), lb = video_load16(yb);
        a[0] = la.x; a[1] = la.y; a[2] = la.z; a[3] = la.w; b[0] = lb.x; b[1] = lb.y; b[2] = lb.z; b[3] = lb.w;
        uint2 lu, lv; __builtin_memcpy(&lu, up, 8); __builtin_memcpy(&lv, vp, 8);
        u[0] = lu.x; u[1] = lu.y; v[0] = lv.x; v[1] = lv.y;
    } else {
#pragma unroll
        for (int i = 0; i < VIDEO_RUN; i++) if (i < n) { a[i >> 2] |= (uint32_t)ya[i] << (8*(i & 3)); b[i >> 2] |= (uint32_t)yb[i] << (8*(i & 3)); }
#pragma unroll
        for (int i = 0; i < VIDEO_RUN/2; i++) if (2*i < n) { u[i >> 2] |= (uint32_t)up[i] << (8*(i & 3)); v[i >> 2] |= (uint32_t)vp[i] << (8*(i & 3)); }
    }
    uint32_t ra[12], rb[12];
    video_convert_run(a, u, v, ra);
    video_convert_run(b, u, v, rb);
    if (n == VIDEO_RUN && w % VIDEO_RUN == 0) {                         // every row starts on a 16-byte boundary: three aligned stores per row
#pragma unroll
        for (int k = 0; k < 3; k++) {
            reinterpret_cast<uint4*>(oa)[k] = make_uint4(ra[4*k], ra[4*k + 1], ra[4*k + 2], ra[4*k + 3]);
            reinterpret_cast<uint4*>(ob)[k] = make_uint4(rb[4*k], rb[4*k + 1], rb[4*k + 2], rb[4*k + 3]);
        }
    } else if (n == VIDEO_RUN) {
        __builtin_memcpy(oa, ra, 48); __builtin_memcpy(ob, rb, 48);
    } else {
#pragma unroll
        for (int i = 0; i < 3*VIDEO_RUN; i++) if (i < 3*n) { oa[i] = (uint8_t)(ra[i >> 2] >> (8*(i & 3))); ob[i] = (uint8_t)(rb[i >> 2] >> (8*(i & 3))); }
    }
}

// One launch serves one frame: FORMAT is SFX_VIDEO_RGB24 (0) or SFX_VIDEO_I420 (1)
template <int FORMAT> __global__ __launch_bounds__(VIDEO_THREADS) void k_video_frame(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h) {
    if (FORMAT == 0) video_frame_rgb24(src, dst, w, h); else video_frame_i420(src, dst, w, h);
}
// lanes a frame needs (the launch rounds them up to whole blocks)
inline long video_frame_lanes(int format, int w, int h) {
    return format == 0 ? (long)((3L*w)/16 + 2)*h : (long)((w + VIDEO_RUN - 1)/VIDEO_RUN)*(h/2);
}

}  // namespace sf
