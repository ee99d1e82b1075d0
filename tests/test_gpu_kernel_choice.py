"""
Which kernel instance a visualizer launch gets, pinned row by row: the strip unit's first-fit walk over its instances
(launch_visualizer_strip.hip launch_visualizer_fast), the tiled unit's choice between its shapes (launch_visualizer_tiled.hip
launch_visualizer_tiled) and the generic kernels behind them, through sfx_last_kernel.

TABLE was recorded on the commit BEFORE the choice moved out of capi.hip into the two pickers; the pickers must reproduce it string
for string. It is data, never regenerated from the code under test: a deliberate change of a threshold or of the order of the
instances edits the rows it moves, by hand, with the reason.

The choice depends on texels per sample and on a block's window in cells, so backgrounds scaled with the output reach the same rows
as the full sizes do (no output here is larger than 640 x 360). Covered: the ten strip instances, the four tiled render shapes, the
twelve tiled fused shapes with the ones sized per launch at 2x and at 4x, the generic kernels for windows no tile holds and for a
background the tiles do not apply to (float texels); identity, zoomed / panned, rolled (17, 45, 90 degrees) and tilted cameras;
SHADERFLOW_VIS_FAST unset, 0 and 1 (read at every launch). SHADERFLOW_VIS_SHAPE is read once per process and is not varied here:
which rolled shape wins where only that switch decides (the 128 x 1 and 64 x 2 pixel blocks lose the cost comparison nearly
everywhere) is covered by comparing the unit's device code with the parent's, kernel by kernel, not by this test.
"""
import numpy as np
import pytest

from shaderflow_amd import _native as N
from tests.helpers import Gpu, gpu_bind_all, visualizer_inputs
from tests.test_gpu_pixels import _turn_camera

pytestmark = pytest.mark.gpu

SCREEN = 0          # the samples themselves into an RGBA8 target (sfx_render); 1, 2, 4: fused with the resolve at that factor

CAMERAS = {
    "identity": dict(),
    "zoomed": dict(iCameraZoom=1.3, iCameraPosition=(0.11, -0.07, 0.0)),
    "wide": dict(iCameraZoom=0.8),
    "roll17": dict(roll=17.0),
    "roll45": dict(roll=45.0),
    "roll90": dict(roll=90.0),
    "tilted": dict(roll=10.0, tilt=12.0),
    "tilt40": dict(tilt=40.0),          # the one camera found that leaves the 64 x 8 block's window too large and the 128 x 2 block's inside its tile
    "zoom0.34": dict(iCameraZoom=0.34),   # (with 1145 background rows: a window 16 sample rows overflow and 8 do not)
}

# (width, height, SCREEN or ssaa, background (width, height[, "float"]), camera, SHADERFLOW_VIS_FAST, sfx_last_kernel)
TABLE = [
    (160, 90, SCREEN, (768, 432), "identity", None, "k_render<PlainShader<2>>"),
    (320, 180, SCREEN, (384, 216), "roll17", 0, "k_render<PlainShader<2>>"),
    (64, 36, SCREEN, (256, 144), "zoomed", 1, "k_render<PlainShader<2>>"),
    (200, 48, SCREEN, (192, 108), "identity", None, "k_render<VisualizerShader<0, 0, 1>>"),
    (640, 360, SCREEN, (1536, 864), "roll90", None, "k_render<VisualizerShader<0, 0, 1>>"),
    (160, 90, SCREEN, (256, 144), "zoomed", 0, "k_render<VisualizerShader<0, 0, 1>>"),
    (320, 180, SCREEN, (512, 288), "identity", None, "k_render<VisualizerShader<0, 0, 4, 1, 1, 128, 64, 8>>"),
    (64, 36, SCREEN, (48, 27), "roll17", 1, "k_render<VisualizerShader<0, 0, 4, 1, 1, 128, 64, 8>>"),
    (200, 48, SCREEN, (32, 18), "roll45", None, "k_render<VisualizerShader<0, 0, 4, 1, 1, 128, 64, 8>>"),
    (640, 360, SCREEN, (48, 27), "tilt40", None, "k_render<VisualizerShader<128, 10, 1>>"),
    (640, 360, SCREEN, (16, 9), "roll17", 0, "k_render<VisualizerShader<64, 15, 6, 1, 1, 128, 64, 8>>"),
    (160, 90, SCREEN, (16, 9), "tilted", None, "k_render<VisualizerShader<64, 15, 6, 1, 1, 128, 64, 8>>"),
    (320, 180, SCREEN, (16, 9), "zoomed", 0, "k_render<VisualizerShader<64, 15, 6, 1, 1, 128, 64, 8>>"),
    (128, 360, SCREEN, (64, 1145), "zoom0.34", None, "k_visualizer_strip<66, 15, 1, 1, 6, 1, true>"),
    (320, 180, SCREEN, (16, 9), "identity", None, "k_visualizer_strip<66, 22, 1, 2, 4, 1, true>"),
    (200, 48, SCREEN, (16, 9), "wide", None, "k_visualizer_strip<66, 22, 1, 2, 4, 1, true>"),
    (64, 36, SCREEN, (16, 9), "zoomed", 1, "k_visualizer_strip<66, 22, 1, 2, 4, 1, true>"),
    (64, 36, 1, (320, 180), "identity", None, "k_render_resolve<PlainShader<2>, 1>"),
    (640, 360, 1, (512, 288), "roll45", None, "k_render_resolve<PlainShader<2>, 1>"),
    (64, 36, 1, (384, 216), "wide", None, "k_render_resolve<PlainShader<2>, 1>"),
    (64, 36, 1, (80, 45), "identity", None, "k_render_resolve<VisualizerShader<0, 0, 4>, 1>"),
    (64, 36, 1, (16, 9), "roll90", None, "k_render_resolve<VisualizerShader<0, 0, 4>, 1>"),
    (64, 36, 1, (96, 54), "wide", None, "k_render_resolve<VisualizerShader<0, 0, 4>, 1>"),
    (640, 360, 1, (16, 9), "identity", None, "k_render_resolve<VisualizerShader<128, 10, 1>, 1>"),
    (160, 90, 1, (16, 9), "tilted", None, "k_render_resolve<VisualizerShader<128, 10, 1>, 1>"),
    (64, 36, 1, (16, 9), "wide", None, "k_render_resolve<VisualizerShader<128, 10, 1>, 1>"),
    (160, 90, 2, (2048, 1152), "identity", None, "k_render_resolve<PlainShader<2>, 2>"),
    (320, 180, 2, (1536, 864), "roll17", 1, "k_render_resolve<PlainShader<2>, 2>"),
    (64, 36, 2, (768, 432), "zoomed", 1, "k_render_resolve<PlainShader<2>, 2>"),
    (320, 180, 2, (1536, 864), "identity", None, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 32>, 2>"),
    (64, 36, 2, (160, 90), "roll17", 0, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 32>, 2>"),
    (200, 48, 2, (384, 216), "zoomed", 1, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 32>, 2>"),
    (64, 36, 2, (256, 144), "identity", None, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 64>, 2>"),
    (64, 36, 2, (256, 144), "roll90", None, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 64>, 2>"),
    (200, 48, 2, (256, 144), "zoomed", 0, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 64>, 2>"),
    (200, 48, 2, (64, 36), "roll17", 1, "k_render_resolve<VisualizerShader<0, 0, 4, 4, 4, 32>, 2>"),
    (160, 90, 2, (48, 27), "roll45", None, "k_render_resolve<VisualizerShader<0, 0, 4, 4, 4, 32>, 2>"),
    (640, 360, 2, (320, 180), "tilted", None, "k_render_resolve<VisualizerShader<0, 0, 4, 4, 4, 32>, 2>"),
    (64, 36, 2, (120, 68), "identity", None, "k_render_resolve<VisualizerShader<0, 0, 4>, 2>"),
    (320, 180, 2, (768, 432), "wide", None, "k_render_resolve<VisualizerShader<0, 0, 4>, 2>"),
    (160, 90, 2, (160, 90), "zoomed", 0, "k_render_resolve<VisualizerShader<0, 0, 4>, 2>"),
    (64, 36, 2, (160, 90), "roll90", None, "k_render_resolve<VisualizerShader<0, 0, 8, 1, 2, 64>, 2>"),
    (320, 180, 2, (512, 288), "roll17", 0, "k_render_resolve<VisualizerShader<0, 0, 8, 1, 4, 32>, 2>"),
    (200, 48, 2, (120, 68), "roll45", None, "k_render_resolve<VisualizerShader<0, 0, 8, 1, 4, 32>, 2>"),
    (64, 36, 2, (48, 27), "tilted", None, "k_render_resolve<VisualizerShader<0, 0, 8, 1, 4, 32>, 2>"),
    (64, 36, 2, (48, 27), "identity", 0, "k_render_resolve<VisualizerShader<64, 11, 8, 1, 2, 64>, 2>"),
    (160, 90, 2, (48, 27), "roll17", 1, "k_render_resolve<VisualizerShader<64, 11, 8, 1, 2, 64>, 2>"),
    (320, 180, 2, (192, 108), "zoomed", 1, "k_render_resolve<VisualizerShader<64, 11, 8, 1, 2, 64>, 2>"),
    (200, 48, 2, (16, 9), "identity", 0, "k_render_resolve<VisualizerShader<80, 10, 8>, 2>"),
    (320, 180, 2, (16, 9), "roll17", 1, "k_render_resolve<VisualizerShader<80, 10, 8>, 2>"),
    (200, 48, 2, (48, 27), "zoomed", 1, "k_render_resolve<VisualizerShader<80, 10, 8>, 2>"),
    (160, 90, 2, (16, 9), "identity", 1, "k_visualizer_fast<72, 10, 128, 8>"),
    (640, 360, 2, (16, 9), "zoomed", 1, "k_visualizer_fast<72, 10, 128, 8>"),
    (320, 180, 2, (256, 144), "identity", None, "k_visualizer_strip<120, 13, 2, 6, 4, 4, true>"),
    (64, 36, 2, (64, 36), "wide", None, "k_visualizer_strip<120, 13, 2, 6, 4, 4, true>"),
    (200, 48, 2, (48, 27), "zoomed", None, "k_visualizer_strip<120, 13, 2, 6, 4, 4, true>"),
    (640, 360, 2, (16, 9), "identity", None, "k_visualizer_strip<72, 12, 2, 9, 6, 4, false>"),
    (160, 90, 2, (16, 9), "wide", None, "k_visualizer_strip<72, 12, 2, 9, 6, 4, false>"),
    (320, 180, 2, (16, 9), "zoomed", None, "k_visualizer_strip<72, 12, 2, 9, 6, 4, false>"),
    (64, 36, 2, (80, 45), "identity", None, "k_visualizer_strip<92, 16, 2, 3, 4, 2, true>"),
    (200, 48, 2, (120, 68), "wide", None, "k_visualizer_strip<92, 16, 2, 3, 4, 2, true>"),
    (640, 360, 2, (640, 360), "zoomed", None, "k_visualizer_strip<92, 16, 2, 3, 4, 2, true>"),
    (200, 48, 4, (1024, 576), "identity", None, "k_render_resolve<PlainShader<2>, 4>"),
    (640, 360, 4, (2048, 1152), "roll17", 0, "k_render_resolve<PlainShader<2>, 4>"),
    (160, 90, 4, (1536, 864), "zoomed", 1, "k_render_resolve<PlainShader<2>, 4>"),
    (640, 360, 4, (2048, 1152), "identity", None, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 32>, 4>"),
    (160, 90, 4, (192, 108), "roll17", 0, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 32>, 4>"),
    (320, 180, 4, (1024, 576), "zoomed", 1, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 32>, 4>"),
    (160, 90, 4, (512, 288), "identity", None, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 64>, 4>"),
    (640, 360, 4, (640, 360), "roll17", 1, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 64>, 4>"),
    (64, 36, 4, (160, 90), "zoomed", 0, "k_render_resolve<VisualizerShader<0, 0, 4, 1, 1, 64>, 4>"),
    (64, 36, 4, (160, 90), "identity", None, "k_render_resolve<VisualizerShader<0, 0, 4>, 4>"),
    (640, 360, 4, (320, 180), "roll90", None, "k_render_resolve<VisualizerShader<0, 0, 4>, 4>"),
    (200, 48, 4, (160, 90), "zoomed", 1, "k_render_resolve<VisualizerShader<0, 0, 4>, 4>"),
    (640, 360, 4, (512, 288), "identity", 0, "k_render_resolve<VisualizerShader<56, 14, 6, 1, 4, 32>, 4>"),
    (64, 36, 4, (32, 18), "roll17", 1, "k_render_resolve<VisualizerShader<56, 14, 6, 1, 4, 32>, 4>"),
    (200, 48, 4, (64, 36), "zoomed", 0, "k_render_resolve<VisualizerShader<56, 14, 6, 1, 4, 32>, 4>"),
    (160, 90, 4, (16, 9), "identity", 0, "k_render_resolve<VisualizerShader<80, 10, 6>, 4>"),
    (200, 48, 4, (16, 9), "roll17", 1, "k_render_resolve<VisualizerShader<80, 10, 6>, 4>"),
    (640, 360, 4, (16, 9), "zoomed", 0, "k_render_resolve<VisualizerShader<80, 10, 6>, 4>"),
    (640, 360, 4, (16, 9), "identity", None, "k_visualizer_strip<20, 13, 4, 10, 6, 2, false>"),
    (320, 180, 4, (16, 9), "wide", None, "k_visualizer_strip<20, 13, 4, 10, 6, 2, false>"),
    (160, 90, 4, (16, 9), "zoomed", 1, "k_visualizer_strip<20, 13, 4, 10, 6, 2, false>"),
    (64, 36, 4, (48, 27), "identity", None, "k_visualizer_strip<40, 13, 4, 10, 6, 2, false>"),
    (640, 360, 4, (640, 360), "wide", None, "k_visualizer_strip<40, 13, 4, 10, 6, 2, false>"),
    (200, 48, 4, (48, 27), "zoomed", 1, "k_visualizer_strip<40, 13, 4, 10, 6, 2, false>"),
    (640, 360, 4, (768, 432), "identity", None, "k_visualizer_strip<40, 14, 4, 6, 8, 2, false>"),
    (320, 180, 4, (512, 288), "wide", None, "k_visualizer_strip<40, 14, 4, 6, 8, 2, false>"),
    (640, 360, 4, (640, 360), "zoomed", 1, "k_visualizer_strip<40, 14, 4, 6, 8, 2, false>"),
    (200, 48, 4, (128, 72), "identity", None, "k_visualizer_strip<56, 16, 4, 6, 6, 2, false>"),
    (160, 90, 4, (320, 180), "wide", None, "k_visualizer_strip<56, 16, 4, 6, 6, 2, false>"),
    (640, 360, 4, (768, 432), "zoomed", 1, "k_visualizer_strip<56, 16, 4, 6, 6, 2, false>"),
    # a background the tiles do not apply to: float texels
    (96, 54, SCREEN, (48, 27, "float"), "identity", None, "k_render<PlainShader<2>>"),
    (96, 54, 2, (48, 27, "float"), "identity", None, "k_render_resolve<PlainShader<2>, 2>"),
    (96, 54, 4, (48, 27, "float"), "identity", None, "k_render_resolve<PlainShader<2>, 4>"),
]


@pytest.fixture()
def gpu():
    g = Gpu()
    yield g
    g.close()


@pytest.mark.parametrize("w,h,mode,bg,camera,fast,kernel", TABLE)
def test_visualizer_kernel_choice(gpu, monkeypatch, w, h, mode, bg, camera, fast, kernel):
    u, arrays, params = visualizer_inputs(w, h, seed=7, volume=0.8, bg_size=bg[:2])
    if len(bg) > 2:
        arrays["background"] = (arrays["background"].astype(np.float32)/255.0).astype(np.float32)
    _turn_camera(u, **CAMERAS[camera])
    u.iSSAA = float(mode or 1)
    prog, _ = gpu.program("visualizer")
    gpu.set_uniforms(prog, u)
    gpu_bind_all(gpu, prog, arrays, params)
    if fast is None:
        monkeypatch.delenv("SHADERFLOW_VIS_FAST", raising=False)
    else:
        monkeypatch.setenv("SHADERFLOW_VIS_FAST", str(fast))
    if mode == SCREEN:
        N.check(gpu.lib.sfx_render(prog, gpu.empty(w, h, 4), 0))
    else:
        N.check(gpu.lib.sfx_render_resolve(prog, gpu.empty(w, h, 3), mode, 1 if mode == 1 else 2))
    assert gpu.lib.sfx_last_kernel().decode() == kernel
