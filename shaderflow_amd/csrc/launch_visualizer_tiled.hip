// launch_visualizer_tiled.hip — visualizer.frag over an LDS tile of background cells, one sample per lane (visualizer_kernels.hpp
// VisualizerShader: round 1's kernels): what runs under rolled / tilted cameras and for windows no table-driven kernel takes. The
// choice between the shapes is made HERE, by launch_visualizer_tiled at the end of the file: every shape is written once, as the
// type beside its launch, and the extents of its block and of its tile come from that type. One of the launch units of
// libshaderflow_hip.so (launch.hpp).
#include "launch.hpp"
#include "launch_geometry.hpp"
#include "launch_templates.hpp"
#include "visualizer_kernels.hpp"

#include <cstdlib>

using namespace sf;

namespace sfl {
namespace {

// the cells of a fixed tile, from the shape's type
template <class SHADER> struct Tile;
template <int PITCH, int ROWS, int... REST> struct Tile<VisualizerShader<PITCH, ROWS, REST...>> { static constexpr int pitch = PITCH, rows = ROWS; };

struct Window {                                                       // of one block, in cells (launch_geometry.hpp)
    int tw = 0, th = 0;
    size_t lds() const { return (size_t)tw*th*48; }
    template <class SHADER> bool in_tile() const { return tw <= Tile<SHADER>::pitch && th <= Tile<SHADER>::rows; }
    void odd_pitch() { tw |= 1; }
};
static Window window_of(const RenderArgs& a, int sx, int sy) { Window w; visualizer_window_bound(a, sx, sy, w.tw, w.th); return w; }
// what a block of SHADER shades: BLOCK_W x BLOCK_H samples of k_render, BLOCK_PX x FUSED_ROWS*THREAD_ROWS pixels of k_render_resolve at 2x / 4x
template <class SHADER> static Window fused_window(const RenderArgs& a, int ssaa) { return window_of(a, SHADER::BLOCK_PX*ssaa, SHADER::FUSED_ROWS*SHADER::THREAD_ROWS*ssaa); }

static RenderArgs with_tile(const RenderArgs& a, const Window& w) { RenderArgs d = a; d.tile_pitch = w.tw; d.tile_rows = w.th; return d; }   // a tile sized per launch
static int launched(int rc) { return rc < 0 ? rc : 1; }
// (`ALLOWED`: the supersampling factors the shape is compiled for, launch_templates.hpp)
template <class SHADER, int... ALLOWED> static int fused_sized(const RenderArgs& a, const Window& w, int ssaa, int frames, hipStream_t s) {
    return launched(launch_fused_s<SHADER, ALLOWED...>(with_tile(a, w), ssaa, frames, s, w.lds()));
}
// a fixed tile at S: 1 when the window fits it and the launch went out
template <class SHADER, int S> static int fused_fixed(const RenderArgs& a, const Window& w, int frames, hipStream_t s) {
    return w.in_tile<SHADER>() ? launched(launch_fused_s<SHADER, S>(a, S, frames, s)) : 0;
}

using Row2 = VisualizerShader<128, 10, 1>;                            // 128 x 2 samples (k_render) or pixels (fused, no supersampling) over 128 x 10 cells

// ---- the samples themselves into a target (k_render): a fixed tile, or one sized per launch for the same block ----
template <class FIXED, class SIZED> static int render_pair(const RenderArgs& a, size_t lds_limit, int frames, hipStream_t s) {
    static_assert(FIXED::BLOCK_W == SIZED::BLOCK_W && FIXED::BLOCK_H == SIZED::BLOCK_H, "one window serves both");
    const Window w = window_of(a, FIXED::BLOCK_W, FIXED::BLOCK_H);
    if (w.tw <= 0) return 0;
    if (w.in_tile<FIXED>()) { launch_render_t<FIXED>(a, frames, s); return 1; }
    if (w.lds() <= lds_limit) { launch_render_t<SIZED>(with_tile(a, w), frames, s, w.lds()); return 1; }
    return 0;
}
static int pick_render(const RenderArgs& a, int frames, hipStream_t s) {
    // first choice: 64 x 8 samples per block over a 64 x 15 tile — three 512-thread blocks per CU and two staged cells per
    // sample, against two 256-thread blocks and five cells for the 128 x 2 shape (1080p without SSAA: 8.4 -> see DESIGN §7)
    // sparser outputs (720p over a 1080-row background: 1.3 texels per sample): the same block shape over a tile sized per
    // launch, as long as two blocks share a CU — the 128 x 2 shape would need a 174 x 11 window there (one 256-thread block per CU)
    if (const int rc = render_pair<VisualizerShader<64, 15, 6, 1, 1, 128, 64, 8>, VisualizerShader<0, 0, 4, 1, 1, 128, 64, 8>>(a, 76*1024, frames, s)) return rc;
    return render_pair<Row2, VisualizerShader<0, 0, 1>>(a, VIS_LDS_LIMIT, frames, s);      // (a window wider than the fixed tile: sized per launch)
}

// ---- fused with the resolve (k_render_resolve) ----
// no supersampling: the fused kernel covers 128 x 2 pixels per block whatever the shape's BLOCK_PX and rows say (launch_templates.hpp
// launch_fused_s) — NOT derivable from the type, so the two numbers stand here
static int pick_fused_1x(const RenderArgs& a, int frames, hipStream_t s) {
    const Window w = window_of(a, 128, 2);
    if (const int rc = fused_fixed<Row2, 1>(a, w, frames, s)) return rc;
    return w.lds() <= VIS_LDS_LIMIT ? fused_sized<VisualizerShader<0, 0, 4>, 1>(a, w, 1, frames, s) : 0;
}
template <class SHADER, int S> static int try_fixed(const RenderArgs& a, int frames, hipStream_t s) { return fused_fixed<SHADER, S>(a, fused_window<SHADER>(a, S), frames, s); }

// A rolled or tilted camera at 2x: a block's window grows with the block's extent along BOTH axes, so squarer blocks stage fewer cells
// per pixel (C3 rolled by 45 degrees: 64 x 2 pixels see 31 x 31 cells, 32 x 4 see 23 x 23) (round 5: and quads that WALK two or four
// rows — one sample per lane left every per-block cost, the camera's ray, the window and the staging, 56 % of a rolled launch, to be
// paid per sample). The cheapest of the candidates wins: cells staged per pixel + what a block pays once per LANE (ray set-up, window,
// barriers), ROLLED_LANE_COST cells' worth.
constexpr float ROLLED_LANE_COST = 2.0f;
struct Sized {                                                        // the tile sized per launch that a loop over candidates settled on
    int (*launch)(const RenderArgs&, const Window&, int, int, hipStream_t) = nullptr;
    Window w;
    float cost = 0.0f;
};
static int rolled_only() {                                            // A/B switch for measurements: the one candidate to try, read once
    static const int only = [] { const char* e = getenv("SHADERFLOW_VIS_SHAPE"); return e ? atoi(e) : -1; }();
    return only;
}
template <class SHADER> static void rolled_candidate(const RenderArgs& a, int k, Sized& best) {
    if (rolled_only() >= 0 && k != rolled_only()) return;
    Window w = fused_window<SHADER>(a, 2);
    // an odd pitch: a cell is 12 dwords, and with the camera turned by a quarter the lanes of a wave read down a COLUMN of cells —
    // 16 cells per row put every one of them on the same banks (730 -> 448 frames/s at C3, 90 degrees).
    // (made odd BEFORE the LDS test: what is checked is what is launched)
    w.odd_pitch();
    if (w.lds() > 72*1024) return;                                   // two 512-thread blocks per CU at least
    const float cost = (float)w.tw*(float)w.th/(float)(SHADER::BLOCK_PX*SHADER::THREAD_ROWS*SHADER::FUSED_ROWS) + ROLLED_LANE_COST/(float)SHADER::FUSED_ROWS;
    if (!best.launch || cost < best.cost) best = {&fused_sized<SHADER, 2>, w, cost};
}

// Denser backgrounds (1080p output at 2x SSAA over a 1080-row background: 0.43 texel per sample; backgrounds larger than the
// output): the tile is sized per launch in dynamic LDS, and the block narrows from 128 to 64 or 32 pixels until its window leaves
// room for at least two blocks per CU. True when the search ends with this width.
template <class SHADER> static bool narrowed(const RenderArgs& a, int ssaa, Sized& best) {
    Window w = fused_window<SHADER>(a, ssaa);
    w.odd_pitch();                                                    // (see above), before the LDS test
    if (w.lds() > VIS_LDS_LIMIT) return false;
    best = {&fused_sized<SHADER, 2, 4>, w};
    return w.lds() <= 64*1024;
}

static int pick_fused(const RenderArgs& a, int ssaa, int frames, hipStream_t s) {
    if (ssaa == 1) return pick_fused_1x(a, frames, s);
    int rc = 0;
    if (ssaa == 2) {
        if ((rc = try_fixed<VisualizerShader<80, 10, 8, 1, 1, 128>, 2>(a, frames, s))) return rc;
        // 0.43 texel per sample (1080p output at 2x SSAA over a 1080-row background): 64 pixels x 2 rows per block see a 63 x 10
        // window — a 64 x 11 tile (33 KB) keeps four 512-thread blocks on a CU, where the tile sized per launch below holds two
        if ((rc = try_fixed<VisualizerShader<64, 11, 8, 1, 2, 64>, 2>(a, frames, s))) return rc;
    } else {
        // four samples per lane need more registers: 6 waves per SIMD without spills beat 8 with (8K 4xSSAA: 55 -> 63 frames/s)
        if ((rc = try_fixed<VisualizerShader<80, 10, 6, 1>, 4>(a, frames, s))) return rc;
        // the same for 4x SSAA at 0.2-0.3 texel per sample (1080p / 720p outputs): 32 pixels x 4 rows per block, a 56 x 14 tile (37 KB)
        if ((rc = try_fixed<VisualizerShader<56, 14, 6, 1, 4, 32>, 4>(a, frames, s))) return rc;
    }
    using Px128 = VisualizerShader<0, 0, 4, 1, 1, 128>;               // (a candidate of both searches below)
    Sized best;
    if (ssaa == 2 && !a.identity_camera && !a.axis_camera) {
        // (measured at C3, 17 / 45 degrees: 32 x 4 x 1: 684 / 662 frames/s, 32 x 4 x 4: 743 / 663; the two-row walks and the
        // 64-wide ones spill or leave blocks off their tile and lose: profiles/r05_rolled_camera.txt)
        // (64 x 2 and 32 x 4: eight waves per SIMD, not the four of the other tiles sized per launch: 555 -> 696 frames/s at C3 rolled by 17 degrees)
        rolled_candidate<Px128>(a, 0, best);
        rolled_candidate<VisualizerShader<0, 0, 8, 1, 2, 64>>(a, 1, best);
        rolled_candidate<VisualizerShader<0, 0, 8, 1, 4, 32>>(a, 2, best);
        rolled_candidate<VisualizerShader<0, 0, 4, 4, 4, 32>>(a, 3, best);
        if (best.launch) return best.launch(a, best.w, ssaa, frames, s);
    }
    (void)(narrowed<Px128>(a, ssaa, best) || narrowed<VisualizerShader<0, 0, 4, 1, 1, 64>>(a, ssaa, best) || narrowed<VisualizerShader<0, 0, 4, 1, 1, 32>>(a, ssaa, best));
    return best.launch ? best.launch(a, best.w, ssaa, frames, s) : 0;
}

}  // namespace

int launch_visualizer_tiled(const RenderArgs& a, int ssaa, int frames, hipStream_t s, bool to_screen) {
    if (!visualizer_tile_applicable(a.tex[TEX_BACKGROUND])) return 0;
    return to_screen ? pick_render(a, frames, s) : pick_fused(a, ssaa, frames, s);
}

}  // namespace sfl
