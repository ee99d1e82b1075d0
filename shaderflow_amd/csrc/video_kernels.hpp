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
//
// k_video_planar: every other planar layout (SFX_VIDEO_PLANAR, sfx_video_create_planar) → the same texture. NORMATIVE, and like the
// above this project's own definition, unpinned against swscale. A LAYOUT has five parts:
//   subsampling   420, 422, 444 or mono            depth b   8, 10 or 12
//   matrix        bt601, bt709 or bt2020 (non-constant luminance)          range   limited or full
//   chroma filter nearest or linear, with a horizontal siting of centre or left
// A frame is planes Y, Cb, Cr, top row first. 8-bit samples are bytes; deeper samples are little-endian 16-bit words, and a word above
// 2^b - 1 counts as 2^b - 1. mono has only Y. Chroma planes are (w/2 x h/2) for 420, (w/2 x h) for 422, (w x h) for 444. A subsampled
// axis needs an even extent; 444 and mono take any extents >= 1.
//
// Coefficients. Kr, Kb = .299/.114 (bt601), .2126/.0722 (bt709), .2627/.0593 (bt2020); Kg = 1 - Kr - Kb.
//   limited: ys = 255/(219 2^(b-8)), cs = 255/(224 2^(b-8)), luma offset 16 2^(b-8)        full: ys = cs = 255/(2^b - 1), offset 0
// The chroma midpoint is 2^(b-1). The five integers are floor(x 2^S + 1/2) of
//   cy = ys    crv = 2(1-Kr) cs    cgu = 2(1-Kb) Kb/Kg cs    cgv = 2(1-Kr) Kr/Kg cs    cbu = 2(1-Kb) cs
// with S = 8 for b = 8, 14 for b = 10 and 16 for b = 12 (8-bit bt601 limited: 298, 409, 100, 208, 516 — the constants above; every
// intermediate below fits a signed 32-bit word). The host builds them (capi_video.hip: planar_coefficients).
//
// Chroma is carried in SIXTEENTHS with no rounding of its own: C16 = sum of wy wx c over at most 2 x 2 chroma samples, indices clamped
// to the plane, wy and wx in quarters. Along a subsampled axis, for output position 2i / 2i + 1:
//   nearest          4 on c[i]                      / 4 on c[i]
//   linear, centre   (1, 3) on (c[i-1], c[i])       / (3, 1) on (c[i], c[i+1])
//   linear, left     4 on c[i]                      / (2, 2) on (c[i], c[i+1])
// Vertical linear is the centre rule (420 only); a non-subsampled axis has weight 4 on its own sample.
// D16 = Cb16 - 16 mid, E16 = Cr16 - 16 mid.
//
// One rounding per value. With C = Y - offset and H = 1 << (S+3), arithmetic shifts:
//   R = clip8((16 cy C + crv E16 + H) >> (S+4))
//   G = clip8((16 cy C - cgu D16 - cgv E16 + H) >> (S+4))
//   B = clip8((16 cy C + cbu D16 + H) >> (S+4))                    mono: R = G = B from the Y term
// For 8-bit 420 bt601 limited nearest this is the I420 formula bit for bit ((16a + 2048) >> 12 == (a + 128) >> 8); that layout keeps
// k_video_frame<SFX_VIDEO_I420>. tests/planar_ref.py restates all of it in numpy.
//
// The same discipline as the I420 path: a lane takes a run of 16 pixels — on two rows for 420, so that a chroma sample's own row is
// loaded once, on one row otherwise — with 16-byte loads (unaligned where the pitch makes them so), three aligned uint4 stores per row
// when w % 16 == 0, unaligned vector stores for whole runs otherwise and the row's last short run byte by byte. linear also loads the
// chroma sample on either side of the run, and for 420 the chroma row above and below, clamped. No LDS, no atomics.
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

// ---- k_video_planar: the general planar layouts (the header comment defines them) -------------------------------------------------------

enum { PLANAR_420 = 0, PLANAR_422 = 1, PLANAR_444 = 2, PLANAR_MONO = 3 };                  // sfx_planar_layout.subsampling
struct VideoPlanarParams { int cy, crv, cgu, cgv, cbu, offset, mid, shift, depth, siting; };   // shift: S; siting: 0 centre, 1 left

// sample `index` of a plane or row that starts at `plane` (deep samples: 2-byte aligned, every plane and row starts on an even byte)
template <int BPS> __device__ __forceinline__ int planar_sample(const uint8_t* plane, long index, int top) {
    if (BPS == 1) return (int)plane[index];
    const int v = (int)reinterpret_cast<const uint16_t*>(plane)[index];
    return v > top ? top : v;
}

// COUNT (8 or 16) consecutive samples from `p` through 16-byte loads (8 bytes for eight 8-bit samples)
template <int BPS, int COUNT> __device__ __forceinline__ void planar_load_run(const uint8_t* p, int top, int* out) {
    uint32_t words[COUNT*BPS/4];
    if (COUNT*BPS == 8) { uint2 v; __builtin_memcpy(&v, p, 8); words[0] = v.x; words[1] = v.y; }
    else {
#pragma unroll
        for (int k = 0; k < COUNT*BPS/16; k++) { const uint4 v = video_load16(p + 16*k); words[4*k] = v.x; words[4*k + 1] = v.y; words[4*k + 2] = v.z; words[4*k + 3] = v.w; }
    }
#pragma unroll
    for (int i = 0; i < COUNT; i++) {
        if (BPS == 1) out[i] = (int)((words[i >> 2] >> (8*(i & 3))) & 255u);
        else { const int v = (int)((words[i >> 1] >> (16*(i & 1))) & 65535u); out[i] = v > top ? top : v; }
    }
}

// clip8(v >> shift) for a shift known only at run time, written as a clamp IN FRONT of a logical shift (0 … 256 2^shift - 1, then >>):
// the same value for every v. An arithmetic shift followed by the clamp is what the compiler turns, two neighbouring bytes at a time,
// into gfx950's packed shift-and-saturate instruction, whose upper result half it then takes to be zero; on the MI355X it was not
// (the last two bytes of a row's run came out as the upper half of a sum). video_clip8's constant shift of 8 never takes that form.
__device__ __forceinline__ uint32_t planar_clip_shift(int v, int shift, int limit) {
    v = v < 0 ? 0 : v;
    v = v > limit ? limit : v;
    return (uint32_t)v >> shift;
}

// The chroma samples ci0 - 1 … ci0 + 8 of one chroma row (`row`: its first byte, `cw` samples), indices clamped to the row → cc[0 … 9]
template <int BPS, int FILTER> __device__ __forceinline__ void planar_chroma_row(const uint8_t* row, int ci0, int cw, bool whole, int top, int (&cc)[10]) {
    if (whole) {                                                       // ci0 … ci0 + 7 lie in the row
        planar_load_run<BPS, 8>(row + (long)ci0*BPS, top, &cc[1]);
        cc[0] = FILTER ? planar_sample<BPS>(row, ci0 > 0 ? ci0 - 1 : 0, top) : cc[1];
        cc[9] = FILTER ? planar_sample<BPS>(row, ci0 + 8 < cw ? ci0 + 8 : cw - 1, top) : cc[8];
    } else {
#pragma unroll
        for (int k = 0; k < 10; k++) { int at = ci0 - 1 + k; at = at < 0 ? 0 : (at > cw - 1 ? cw - 1 : at); cc[k] = planar_sample<BPS>(row, at, top); }
    }
}

// One lane = one run of 16 pixels on source rows 2p and 2p + 1 (420) or on source row p (422, 444, mono). SUB: PLANAR_*; BPS: bytes
// per sample; FILTER: 0 nearest, 1 linear (444 and mono: always 0, the host says so)
template <int SUB, int BPS, int FILTER>
__global__ __launch_bounds__(VIDEO_THREADS) void k_video_planar(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w, int h, VideoPlanarParams q) {
    constexpr int ROWS = SUB == PLANAR_420 ? 2 : 1;
    const int runs = (w + VIDEO_RUN - 1)/VIDEO_RUN;
    const long index = (long)blockIdx.x*VIDEO_THREADS + threadIdx.x;
    if (index >= (long)runs*(h/ROWS)) return;
    const int p = (int)(index/runs), x0 = ((int)(index - (long)p*runs))*VIDEO_RUN;
    const int n = (w - x0) < VIDEO_RUN ? (w - x0) : VIDEO_RUN;          // pixels of this run
    const bool whole = n == VIDEO_RUN;
    const int top = (1 << q.depth) - 1, row0 = p*ROWS;
    const long luma_bytes = (long)w*h*BPS;

    // chroma of the run's rows, vertically blended, in quarters: index k is chroma sample x0/2 - 1 + k (420, 422) or pixel x0 + k (444)
    int uq[ROWS][VIDEO_RUN + 2], vq[ROWS][VIDEO_RUN + 2];
    if (SUB == PLANAR_444) {
        const uint8_t* cb = src + luma_bytes + ((long)row0*w + x0)*BPS;
        const uint8_t* cr = cb + luma_bytes;
        if (whole) { planar_load_run<BPS, VIDEO_RUN>(cb, top, uq[0]); planar_load_run<BPS, VIDEO_RUN>(cr, top, vq[0]); }
        else {
#pragma unroll
            for (int i = 0; i < VIDEO_RUN; i++) { uq[0][i] = i < n ? planar_sample<BPS>(cb, i, top) : 0; vq[0][i] = i < n ? planar_sample<BPS>(cr, i, top) : 0; }
        }
    } else if (SUB != PLANAR_MONO) {
        const int cw = w/2, ch = h/ROWS, ci0 = x0/2;
        const long pitch = (long)cw*BPS;
        const uint8_t* cb = src + luma_bytes;
        const uint8_t* cr = cb + pitch*ch;
        int u[10], v[10];
        planar_chroma_row<BPS, FILTER>(cb + pitch*p, ci0, cw, whole, top, u);
        planar_chroma_row<BPS, FILTER>(cr + pitch*p, ci0, cw, whole, top, v);
        if (SUB == PLANAR_420 && FILTER) {                             // the centre rule: rows 2p / 2p + 1 take (1, 3) of rows (p - 1, p) / (3, 1) of (p, p + 1)
            const int above = p > 0 ? p - 1 : 0, below = p + 1 < ch ? p + 1 : ch - 1;
            int ua[10], va[10], ub[10], vb[10];
            planar_chroma_row<BPS, FILTER>(cb + pitch*above, ci0, cw, whole, top, ua);
            planar_chroma_row<BPS, FILTER>(cr + pitch*above, ci0, cw, whole, top, va);
            planar_chroma_row<BPS, FILTER>(cb + pitch*below, ci0, cw, whole, top, ub);
            planar_chroma_row<BPS, FILTER>(cr + pitch*below, ci0, cw, whole, top, vb);
#pragma unroll
            for (int k = 0; k < 10; k++) {
                uq[0][k] = ua[k] + 3*u[k]; vq[0][k] = va[k] + 3*v[k];
                uq[ROWS - 1][k] = 3*u[k] + ub[k]; vq[ROWS - 1][k] = 3*v[k] + vb[k];
            }
        } else {
#pragma unroll
            for (int r = 0; r < ROWS; r++)
#pragma unroll
                for (int k = 0; k < 10; k++) { uq[r][k] = 4*u[k]; vq[r][k] = 4*v[k]; }
        }
    }
    // horizontal weights in quarters: even pixels (ep, ec) on (c[i-1], c[i]), odd pixels (oc, on) on (c[i], c[i+1])
    int ep = 0, ec = 4, oc = 4, on = 0;
    if (FILTER) { if (q.siting == 0) { ep = 1; ec = 3; oc = 3; on = 1; } else { oc = 2; on = 2; } }
    const int shift = q.shift + 4, half = 1 << (q.shift + 3), mid16 = 16*q.mid, limit = (256 << shift) - 1;

#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        const uint8_t* yp = src + ((long)(row0 + r)*w + x0)*BPS;
        int y[VIDEO_RUN];
        if (whole) planar_load_run<BPS, VIDEO_RUN>(yp, top, y);
        else {
#pragma unroll
            for (int i = 0; i < VIDEO_RUN; i++) y[i] = i < n ? planar_sample<BPS>(yp, i, top) : 0;
        }
        uint32_t out[12];
#pragma unroll
        for (int k = 0; k < 12; k++) out[k] = 0u;
#pragma unroll
        for (int i = 0; i < VIDEO_RUN; i++) {
            const int c = 16*q.cy*(y[i] - q.offset) + half;
            uint32_t rgb[3];
            if (SUB == PLANAR_MONO) rgb[0] = rgb[1] = rgb[2] = planar_clip_shift(c, shift, limit);
            else {
                int d, e;
                if (SUB == PLANAR_444) { d = 16*uq[0][i]; e = 16*vq[0][i]; }
                else if (i & 1) { d = oc*uq[r][(i >> 1) + 1] + on*uq[r][(i >> 1) + 2]; e = oc*vq[r][(i >> 1) + 1] + on*vq[r][(i >> 1) + 2]; }
                else { d = ep*uq[r][i >> 1] + ec*uq[r][(i >> 1) + 1]; e = ep*vq[r][i >> 1] + ec*vq[r][(i >> 1) + 1]; }
                d -= mid16; e -= mid16;
                rgb[0] = planar_clip_shift(c + q.crv*e, shift, limit);
                rgb[1] = planar_clip_shift(c - q.cgu*d - q.cgv*e, shift, limit);
                rgb[2] = planar_clip_shift(c + q.cbu*d, shift, limit);
            }
#pragma unroll
            for (int k = 0; k < 3; k++) { const int b = 3*i + k; out[b >> 2] |= rgb[k] << (8*(b & 3)); }
        }
        uint8_t* o = dst + ((long)(h - 1 - row0 - r)*w + x0)*3;
        if (whole && w % VIDEO_RUN == 0) {                              // every row starts on a 16-byte boundary: three aligned stores
#pragma unroll
            for (int k = 0; k < 3; k++) reinterpret_cast<uint4*>(o)[k] = make_uint4(out[4*k], out[4*k + 1], out[4*k + 2], out[4*k + 3]);
        } else if (whole) {
            __builtin_memcpy(o, out, 48);
        } else {
#pragma unroll
            for (int i = 0; i < 3*VIDEO_RUN; i++) if (i < 3*n) o[i] = (uint8_t)(out[i >> 2] >> (8*(i & 3)));
        }
    }
}
// lanes a planar frame needs
inline long video_planar_lanes(int subsampling, int w, int h) {
    return (long)((w + VIDEO_RUN - 1)/VIDEO_RUN)*(subsampling == PLANAR_420 ? h/2 : h);
}

}  // namespace sf
