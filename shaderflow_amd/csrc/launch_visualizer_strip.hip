// launch_visualizer_strip.hip — the table-driven visualizer kernels (visualizer_fast.hpp): k_visualizer_axes + one instance of
// k_visualizer_strip / k_visualizer_fast per block geometry. One of the launch units of libshaderflow_hip.so (launch.hpp).
#define SF_UNIT_VISUALIZER_TABLES
#include "launch.hpp"
#include "launch_geometry.hpp"
#include "visualizer_fast.hpp"

#include <cstdlib>

using namespace sf;

namespace sfl {

// the tape's per-frame constants and bar heights (visualizer_kernels.hpp): launched from capi.hip's sfx_render_tape as well
void visualizer_consts_frames(const FrameDyn* dyn, int frame0, int nframes, VisualizerConsts* out, hipStream_t s) {
    hipLaunchKernelGGL(k_visualizer_consts, dim3((nframes + 63)/64), dim3(64), 0, s, dyn, frame0, nframes, out);
}
void visualizer_bars(const float* columns, long count, float* bars, hipStream_t s) {
    hipLaunchKernelGGL(k_visualizer_bars, dim3((unsigned)((count + 255)/256)), dim3(256), 0, s, columns, count, bars);
}

// One instance of the fast path. STRIP_S == 0: k_visualizer_fast (a quad of lanes per pixel, 2x SSAA); otherwise
// k_visualizer_strip<PITCH, ROWS, STRIP_S, WALK, WAVES, CG, HALF> (lanes walk strips of their column; 2x or 4x SSAA fused with the
// resolve, or STRIP_S == 1: the samples to an RGBA8 iScreen). HALF: float16 cells in three planes (visualizer_fast.hpp).
template <int PITCH_, int ROWS_, int STRIP_S_, int WALK_, int WAVES_, int CG_ = (STRIP_S_ ? 8/STRIP_S_ : 4), bool HALF_ = (STRIP_S_ == 1)>
struct Strip {
    static constexpr int PITCH = PITCH_, ROWS = ROWS_, STRIP_S = STRIP_S_, WALK = WALK_, WAVES = WAVES_, CG = CG_;
    static constexpr bool HALF = HALF_;
    static constexpr int SSAA = STRIP_S ? STRIP_S : 2;                // the supersampling factor it serves (1: to the screen)
    static constexpr int COLS = STRIP_S ? 64*CG : 256;                // sample columns per block
    static constexpr int BLOCK_ROWS = STRIP_S ? (8/CG)*WALK : 2;      // sample rows per block
};
template <class... INSTANCES> struct Strips {};

// The instances by supersampling factor, in the order they are tried: the first whose tile holds a block's window takes the launch.
// no SSAA: 0.87 texel per sample at 1080p over a 1080-row background — nothing to share along a strip, but the tables, the folded tap
// pairs and the speculated post-processing still apply
using Strips1x = Strips<
    Strip<66, 22, 1, 2, 4, 1>,                  // strips of two rows over 66 x 22 (two blocks per CU)
    Strip<66, 15, 1, 1, 6, 1>>;                 // 64 columns x 8 rows per block over a 66 x 15 tile (three blocks per CU)
// float16 cells: where the lanes of a wave read DIFFERENT cells the kernel is bound by LDS bandwidth and half the bytes win — 1080p 2x
// 7 200 -> 7 970, 1440p 2x 4 480 -> 4 920, 720p 2x 9 430 -> 13 270 frames/s (profiles/r03_variants.txt); at 4K 2x the lanes share
// their cells and plain float32 multiply-adds are cheaper
using Strips2x = Strips<
    // nine rows: the longest strip that stays inside 64 VGPRs (ten spill), +2 % over eight. 6 waves is what the kernel HAS: 51.8 KB of LDS
    // per block = three blocks = six waves per SIMD (78 registers); asking for 8 only made the compiler say so on every build
    Strip<72, 12, 2, 9, 6, 4, false>,
    // denser outputs (1080p or 1440p at 2x SSAA over a 1080-row background: up to 0.43 texel per sample): strips of six rows, the
    // longest whose 120-cell-wide tile still leaves two blocks per CU
    Strip<120, 13, 2, 6, 4, 4, true>,
    // sparser still (720p at 2x SSAA: 0.65 texel per sample): 128 columns x 12 rows per block, strips of three, 92 x 16 tile
    Strip<92, 16, 2, 3, 4, 2, true>,
    Strip<72, 10, 0, 0, 8>>;                    // the quad kernel; SHADERFLOW_VIS_FAST=1 skips the three strips above
using Strips4x = Strips<
    // 8K at 4x over a 1080-row background (0.0625 texel per sample): a block's window is 17 cells wide — on a 20-cell pitch its staging loop
    // has no idle half (round 6's tile sweep, profiles/r06_c4_tile_sweep.txt: 292.0 -> 295.9 frames/s, the same bytes); wider windows
    // (smaller outputs, larger backgrounds) keep the 40-cell pitch
    Strip<20, 13, 4, 10, 6, 2, false>,
    Strip<40, 13, 4, 10, 6, 2, false>,
    Strip<40, 14, 4, 6, 8, 2, false>,           // 1080p at 4x SSAA: the same tile width with strips of six rows
    Strip<56, 16, 4, 6, 6, 2, false>>;          // 720p at 4x SSAA (0.32 texel per sample)
// A/B builds (tools/variants.sh, tools/experiments/c4_tile_sweep.sh): -DVIS_STRIP_TRY_FIRST="20, 13, 4, 10, 6, 2, false" names one more
// instance by its template arguments; it is tried in front of the list of its own factor. Unset, nothing is compiled for it.
#ifdef VIS_STRIP_TRY_FIRST
using StripsFirst = Strips<Strip<VIS_STRIP_TRY_FIRST>>;
#else
using StripsFirst = Strips<>;
#endif

// the tables for an instance, then its kernel
template <class I> static int launch_visualizer_tables_and_kernel(Context* ctx, const RenderArgs& a, int frames, hipStream_t s) {
    constexpr int PITCH = I::PITCH, ROWS = I::ROWS, STRIP_S = I::STRIP_S, WALK = I::WALK, WAVES = I::WAVES, CG = I::CG, COLS = I::COLS, BLOCK_ROWS = I::BLOCK_ROWS;
    constexpr bool HALF = I::HALF;
    VisTables t;
    t.blocks_x = (a.wr + COLS - 1)/COLS; t.blocks_y = (a.hr + BLOCK_ROWS - 1)/BLOCK_ROWS;
    t.block_columns = COLS; t.block_rows = BLOCK_ROWS; t.tile_pitch = PITCH; t.tile_rows = ROWS;
    t.cell_bytes = HALF ? 8 : 48;                                     // float16 cells in three planes where the lanes of a wave read different cells (visualizer_fast.hpp)
    const size_t entries = (size_t)frames*((size_t)a.wr + a.hr)*VIS_ENTRY_QUADS*sizeof(float4);
    const size_t blocks = (size_t)frames*((size_t)t.blocks_x + t.blocks_y)*sizeof(int4);
    // (+ WALK - 1 rows: a strip's rows are loaded at immediate offsets from its first one, past the frame's last row too)
    const size_t ysteps = STRIP_S ? ((size_t)frames*a.hr + (WALK - 1))*10*sizeof(float4) : 0;
    // the pixel tier (visualizer_fast.hpp visualizer_pixel_gains): fused 2x / 4x launches whose bars come as a table; SHADERFLOW_VIS_PIXEL_TIER=0
    // turns it off (A/B measurements, and the tests that compare the two tiers)
    const Tex& sp = a.tex[TEX_SPECTROGRAM];
    const char* tier_env = getenv("SHADERFLOW_VIS_PIXEL_TIER");
    float reach_uv = 0.0f, reach_agluv = 0.0f;
    bool tier = STRIP_S >= 2 && a.tape_bars && sp.height > 0 && !(tier_env && atoi(tier_env) == 0);
    if (tier) {
        // how far a supersample lies from its pixel's centre: (S - 1)/(2S) of the pixel per axis, bounded by 0.3 of its diagonal for S <= 4
        // (0.25 at 2x, 0.375 at 4x … of the HALF diagonal 0.5): in iCamera.gluv units through the axis camera's slopes, and in agluv units
        float slope_x = 1.0f, slope_y = 1.0f;
        if (!a.identity_camera) {
            bool behind = false;
            slope_x = fabsf(camera_along_axis<0>(a.u, 1.0f, a.aspect, behind) - camera_along_axis<0>(a.u, -1.0f, a.aspect, behind))/2.0f;
            slope_y = fabsf(camera_along_axis<1>(a.u, 1.0f, a.aspect, behind) - camera_along_axis<1>(a.u, -1.0f, a.aspect, behind))/2.0f;
        }
        const float px = 2.0f*a.aspect/(float)a.w*slope_x, py = 2.0f/(float)a.h*slope_y;
        const float part = STRIP_S == 2 ? 0.30f : 0.45f;               // of the pixel's diagonal: 0.25 / 0.375 exactly, with a margin
        reach_uv = part*sqrtf(px*px + py*py);
        reach_agluv = part*sqrtf(4.0f/((float)a.w*(float)a.w) + 4.0f/((float)a.h*(float)a.h));
        if (!(reach_uv < 1.0f) || !(reach_uv > 0.0f)) tier = false;   // (a degenerate camera: NaN or nothing to bound)
    }
    const size_t pixel_entries = tier ? (size_t)frames*((size_t)a.w + a.h)*sizeof(float4) : 0;
    const size_t bars2 = tier ? (size_t)frames*sp.height*2*sizeof(float2) : 0;
    const size_t classes = tier ? (size_t)frames*t.blocks_x*t.blocks_y*8 : 0;
    // the strip plan (visualizer_fast.hpp k_visualizer_strip_plan): the float32-cell 2x instances; SHADERFLOW_VIS_STRIP_PLAN=0 launches their
    // in-kernel form (A/B measurements, and the test that holds the two forms to the same bytes)
    using Kernel = VisualizerStrip<PITCH, ROWS, STRIP_S ? STRIP_S : 2, STRIP_S ? WALK : 1, CG, HALF>;
    constexpr bool CAN_PLAN = STRIP_S == 2 && !HALF;
    const char* plan_env = getenv("SHADERFLOW_VIS_STRIP_PLAN");
    const bool planned = CAN_PLAN && !(plan_env && atoi(plan_env) == 0);
    const size_t strips = (size_t)frames*t.blocks_y*Kernel::ROW_GROUPS;
    // (the weight images only where the kernel reads them: VisualizerStrip::PLAN_COLW)
    constexpr bool PLAN_IMAGES = CAN_PLAN && VIS_STRIP_PLAN_COLW && ROWS <= Kernel::COLW_SLOTS;
    const size_t plan_records = planned ? strips*sizeof(int4) : 0, plan_colw = planned && PLAN_IMAGES ? strips*WALK*Kernel::COLW_SLOTS*sizeof(float2) : 0;
    static_assert(!CAN_PLAN || (WALK*Kernel::COLW_SLOTS*sizeof(float2)) % 16 == 0, "what follows the weight images stays 16-byte aligned");
    const size_t needed = entries + blocks + ysteps + plan_records + plan_colw + pixel_entries + bars2 + classes;
    if (ctx->vis_tables_bytes < needed) {
        hipStreamSynchronize(s);
        hipFree(ctx->vis_tables); ctx->vis_tables = nullptr; ctx->vis_tables_bytes = 0;
        if (hipMalloc(&ctx->vis_tables, needed) != hipSuccess) return fail(SFX_E_HIP, "visualizer tables of %d frames: out of device memory", frames);
        ctx->vis_tables_bytes = needed;
    }
    t.columns = (float4*)ctx->vis_tables;
    t.rows = t.columns + (size_t)frames*a.wr*VIS_ENTRY_QUADS;
    t.block_x = (int4*)(t.rows + (size_t)frames*a.hr*VIS_ENTRY_QUADS);
    t.block_y = t.block_x + (size_t)frames*t.blocks_x;
    t.ysteps = STRIP_S ? (float4*)(t.block_y + (size_t)frames*t.blocks_y) : nullptr;
    char* after = (char*)ctx->vis_tables + entries + blocks + ysteps;
    int4* records = planned ? (int4*)after : nullptr;
    float2* images = planned && PLAN_IMAGES ? (float2*)(after + plan_records) : nullptr;
    t.strip_plan = records; t.strip_colw = images;
    after += plan_records + plan_colw;
    t.pixel_columns = tier ? (float4*)after : nullptr;
    t.pixel_rows = tier ? t.pixel_columns + (size_t)frames*a.w : nullptr;
    float2* spread = tier ? (float2*)(after + pixel_entries) : nullptr;
    t.bars2 = spread;
    t.pixel_reach_uv = reach_uv; t.pixel_reach_agluv = reach_agluv;
    uint8_t* wave_classes = tier ? (uint8_t*)(after + pixel_entries + bars2) : nullptr;
    t.wave_classes = wave_classes;
    if (tier) {
        const long count = (long)frames*sp.height*2;
        hipLaunchKernelGGL(k_visualizer_bar_spread, dim3((unsigned)((count + 255)/256)), dim3(256), 0, s, a.tape_bars + (long)a.frame0*a.spectrogram_stride,
                           (long)a.spectrogram_stride, frames, sp.height, sp.repeat_y, spread);
    }
    hipLaunchKernelGGL(k_visualizer_axes, dim3((a.wr + 127)/128 + (a.hr + 127)/128, frames), dim3(128), 0, s, a, t);
    if constexpr (CAN_PLAN) {
        if (planned) {
            const int per_frame = t.blocks_y*Kernel::ROW_GROUPS;      // one wave per strip, four to a block
            hipLaunchKernelGGL((k_visualizer_strip_plan<WALK, Kernel::ROW_GROUPS, Kernel::ROWBYTES, Kernel::COLW_SLOTS>), dim3((per_frame + 3)/4, frames), dim3(256), 0, s, a, t, records, images);
        }
    }
    if constexpr (STRIP_S >= 2) {
        if (tier) {
            const long tiles = (long)t.blocks_x*t.blocks_y*8;
            hipLaunchKernelGGL((k_visualizer_classify<STRIP_S, WALK, CG>), dim3((unsigned)((tiles + 255)/256), frames), dim3(256), 0, s, a, t, wave_classes);
        }
    }
    if constexpr (STRIP_S != 0) {
        g_last_kernel = "k_visualizer_strip<" + std::to_string(PITCH) + ", " + std::to_string(ROWS) + ", " + std::to_string(STRIP_S) + ", " + std::to_string(WALK) + ", " + std::to_string(WAVES) + ", " + std::to_string(CG) + (HALF ? ", true>" : ", false>");
        if constexpr (CAN_PLAN) {
            if (planned) hipLaunchKernelGGL((k_visualizer_strip<PITCH, ROWS, STRIP_S, WALK, WAVES, CG, HALF, true>), dim3(t.blocks_x*t.blocks_y, 1, frames), dim3(512), 0, s, a, t);
            else {
                g_last_kernel += " in-kernel choices";
                hipLaunchKernelGGL((k_visualizer_strip<PITCH, ROWS, STRIP_S, WALK, WAVES, CG, HALF>), dim3(t.blocks_x*t.blocks_y, 1, frames), dim3(512), 0, s, a, t);
            }
        } else hipLaunchKernelGGL((k_visualizer_strip<PITCH, ROWS, STRIP_S, WALK, WAVES, CG, HALF>), dim3(t.blocks_x*t.blocks_y, 1, frames), dim3(512), 0, s, a, t);
    } else {
        g_last_kernel = "k_visualizer_fast<" + std::to_string(PITCH) + ", " + std::to_string(ROWS) + ", 128, " + std::to_string(WAVES) + ">";
        hipLaunchKernelGGL((k_visualizer_fast<PITCH, ROWS, 128, WAVES>), dim3(t.blocks_x*t.blocks_y, 1, frames), dim3(512), 0, s, a, t);
    }
    return 1;
}

// One step of the first-fit walk: the instance launches when the window of its block fits its tile. `plain`: the 2x strips stand aside.
template <class I> static int try_strip(Context* ctx, const RenderArgs& a, int ssaa, int frames, hipStream_t s, bool plain) {
    if (I::SSAA != ssaa || (plain && I::STRIP_S == 2)) return 0;
    int tw = 0, th = 0;
    visualizer_window_bound(a, I::COLS, I::BLOCK_ROWS, tw, th);
    return tw <= I::PITCH && th <= I::ROWS ? launch_visualizer_tables_and_kernel<I>(ctx, a, frames, s) : 0;
}
template <class... I> static int first_fit(Strips<I...>, Context* ctx, const RenderArgs& a, int ssaa, int frames, hipStream_t s, bool plain) {
    int rc = 0;
    (void)(... || ((rc = try_strip<I>(ctx, a, ssaa, frames, s, plain)) != 0));
    return rc;
}

// ---- the fast visualizer path (visualizer_fast.hpp) -----------------------------------------------------------------------
// Identity camera, unorm8 bilinear background, 2x or 4x SSAA, the window of a block inside one of the compiled tiles, and a blur
// whose axis lines fit their slots at the largest radius the launch can see. Returns 1 when it launched, 0 when the configuration
// is not its own (the caller then takes VisualizerShader), < 0 on errors.
int launch_visualizer_fast(Context* ctx, const RenderArgs& a0, int ssaa, int frames, hipStream_t s, bool to_screen) {
    // fused: 2x or 4x SSAA into the RGB8 frame; to_screen: the samples themselves into an RGBA8 iScreen (the two-pass configuration)
    if (to_screen ? (ssaa != 1 || a0.out_dtype != DT_U8 || a0.out_components != 4) : (ssaa != 2 && ssaa != 4)) return 0;
    if (!ctx || !(a0.identity_camera || a0.axis_camera) || !visualizer_tile_applicable(a0.tex[TEX_BACKGROUND])) return 0;
    const char* toggle = getenv("SHADERFLOW_VIS_FAST");              // A/B switch for measurements: 0 = round 1's kernels, 1 = k_visualizer_fast
    if (toggle && atoi(toggle) == 0) return 0;
    const Tex& bg = a0.tex[TEX_BACKGROUND];
    const Tex& sp = a0.tex[TEX_SPECTROGRAM];
    RenderArgs a = a0;
    if (!a.tape_bars) {
        // a bound one-column RG32F spectrogram: the bar heights per texel into the context's scratch (k_visualizer_bars)
        if (a.dyn || a.tape_spectrogram || !sp.data || sp.dtype != DT_F32 || sp.components != 2 || sp.width != 1 || sp.filter != FILTER_NEAREST) return 0;
        const size_t count = (size_t)sp.height*2;
        if (ctx->vis_bars_count < count) {
            hipStreamSynchronize(s);
            hipFree(ctx->vis_bars); ctx->vis_bars = nullptr; ctx->vis_bars_count = 0;
            if (hipMalloc(&ctx->vis_bars, sizeof(float)*count) != hipSuccess) return fail(SFX_E_HIP, "visualizer bar table: out of device memory");
            ctx->vis_bars_count = count;
        }
        visualizer_bars((const float*)sp.data, (long)count, ctx->vis_bars, s);
        a.tape_bars = ctx->vis_bars; a.spectrogram_stride = 0;
    } else if (sp.width != 1 || sp.components != 2) return 0;
    // the axis lines must fit their slots at the largest blur radius of the launch (visualizer_window_bound's conventions)
    const float intensity = a.has_vis ? fabsf(a.vis.intensity) : 0.003f;
    const float ax = intensity*a.bg_scale_x*(float)bg.width;
    const float reach_line = (fabsf(a.tap_x[0]) + 9.0f*fabsf(a.tap_x[1] - a.tap_x[0]))*ax;
    if (!(2.0f*reach_line + 1.0e-3f < (float)(VIS_LINE_CELLS - 1))) return 0;
    const bool plain = toggle && atoi(toggle) == 1;                   // force the quad-per-pixel kernel
    if (const int first = first_fit(StripsFirst{}, ctx, a, ssaa, frames, s, plain)) return first;
    switch (ssaa) {
        case 1: return first_fit(Strips1x{}, ctx, a, ssaa, frames, s, plain);
        case 2: return first_fit(Strips2x{}, ctx, a, ssaa, frames, s, plain);
        default: return first_fit(Strips4x{}, ctx, a, ssaa, frames, s, plain);
    }
}

}  // namespace sfl
