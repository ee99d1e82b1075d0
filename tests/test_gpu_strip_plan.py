"""
The strip kernel's PLAN form (k_visualizer_strip_plan → VisTables::strip_plan; k_visualizer_strip<…, true>): the row lines' new-cell-row
mask, the column line's extent and staged weights, the crossing flag in the diagonal walk's table. No floating-point operation of a sample
differs from the in-kernel form (SHADERFLOW_VIS_STRIP_PLAN=0), so the two forms are held to the SAME BYTES over whole frames — bottom-up and
top_down, through a single launch and through a tape launch of three frames — and one case to the oracle within 1 LSB, so that the plan is
not merely equal to a wrong in-kernel form.

Shapes: the benchmark's density, a quarter of a texel per sample at 2x SSAA, over backgrounds small enough for a frame to take
milliseconds; the instance must be the benchmark's k_visualizer_strip<72, 12, 2, 9, 6, 4, false> (256 sample columns x 18 sample rows per
block, two row groups of nine rows):
    192 x 108 over 96 x 54    1.5 blocks across, whole strips
    192 x 100 over 96 x 50    200 sample rows = 11 blocks of 18 + 2: the last block has a strip of two rows and an empty one
    130 x 55 over 65 x 28     odd width, an odd count of rows in the last strip, a partial column group
Audio states: silence (radius 0: every tap of a line in one cell), a radius just under one texel, the clamp (intensity 0.003, the
benchmark's), and a zoomed and panned axis-aligned camera. The blur's radius in texels is intensity x background height (gtexture scales x
by height/width), so over the small backgrounds above the clamp is 0.16 texel: a line's taps lie in one or two cells. The state "under one
texel" therefore renders each shape's TALL twin — the same width and block structure along y, over a background 320 texels high at a fifth
of a texel per sample, where the clamp's radius is 0.96 texel: the taps of a line spread over three cells, the walk's sides lie two rows of
cells apart and the aligned weights' slots shift along the strip:
    192 x 648 over 96 x 320   whole strips (1 296 sample rows = 72 blocks)
    192 x 640 over 96 x 320   1 280 sample rows = 71 blocks of 18 + 2
    130 x 635 over 65 x 320   1 270 sample rows = 70 blocks + 10: a whole strip and a strip of one row
"""
import os

import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import _native as N
from tests.helpers import Gpu, gpu_bind_all, lsb_report, oracle_textures, usable_cores, visualizer_inputs
from tests.test_gpu_pixels import assert_within_lsb

pytestmark = pytest.mark.gpu
THREADS = usable_cores()
SWITCH = "SHADERFLOW_VIS_STRIP_PLAN"
INSTANCE = "k_visualizer_strip<72, 12, 2, 9, 6, 4, false>"
IN_KERNEL = INSTANCE + " in-kernel choices"                          # what sfx_last_kernel calls the launch without a plan

SHAPES = {"192x108": (192, 108, (96, 54)), "192x100": (192, 100, (96, 50)), "130x55": (130, 55, (65, 28))}
TALL = {"192x108": (192, 648, (96, 320)), "192x100": (192, 640, (96, 320)), "130x55": (130, 635, (65, 320))}
UNDER_ONE_TEXEL = "under one texel"
CAMERA = dict(iCameraZoom=0.8, iCameraPosition=(0.11, -0.07, 0.0))
# iAudioVolume -> intensity = 0.01*clamp(volume^2.5, 0, 0.3): 0 and the clamp (from 0.618 on)
STATES = {"silence": (0.0, None), UNDER_ONE_TEXEL: (0.9, None), "clamp": (0.9, None), "camera": (0.9, CAMERA)}


def shape_of(shape, state):
    return (TALL if state == UNDER_ONE_TEXEL else SHAPES)[shape]


def radius_in_texels(volume, background_height) -> float:
    """visualizer.frag's blur radius over a background of that height: intensity = 0.01*clamp(volume^2.5, 0, 0.3), times the height"""
    return float(np.float32(0.01)*np.float32(min(max(float(volume), 0.0)**2.5, 0.3))*np.float32(background_height))


@pytest.fixture()
def gpu():
    g = Gpu()
    yield g
    g.close()


class switched:
    """The plan switch for the launches inside (the library reads it at every launch)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.get(SWITCH)
        if self.value is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = self.value

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = self.saved


def single_launches(gpu, shape, state, top_down):
    """One frame through sfx_render_resolve with the plan and without: (planned, in-kernel, uniforms, arrays, params)"""
    w, h, bg_size = shape_of(shape, state)
    volume, camera = STATES[state]
    if state == UNDER_ONE_TEXEL:
        assert 0.9 <= radius_in_texels(volume, bg_size[1]) < 1.0, radius_in_texels(volume, bg_size[1])
    u, arrays, params = visualizer_inputs(w, h, seed=43, volume=volume, bg_size=bg_size)
    for key, value in (camera or {}).items():
        cur = getattr(u, key)
        if hasattr(cur, "__len__"):
            for i, v in enumerate(value):
                cur[i] = v
        else:
            setattr(u, key, value)
    u.iSSAA = 2.0
    prog, _ = gpu.program("visualizer")
    gpu.set_uniforms(prog, u)
    gpu_bind_all(gpu, prog, arrays, params)
    N.check(gpu.lib.sfx_ctx_output_top_down(gpu.ctx.handle, int(top_down)))
    try:
        with switched(None):
            planned = gpu.render_resolve(prog, w, h, 2, 2)
            assert gpu.lib.sfx_last_kernel().decode() == INSTANCE, gpu.lib.sfx_last_kernel()
        with switched("0"):
            in_kernel = gpu.render_resolve(prog, w, h, 2, 2)
            assert gpu.lib.sfx_last_kernel().decode() == IN_KERNEL, gpu.lib.sfx_last_kernel()
    finally:
        N.check(gpu.lib.sfx_ctx_output_top_down(gpu.ctx.handle, 0))
    return planned, in_kernel, u, arrays, params


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_single_launch_same_bytes_with_and_without_the_plan(gpu, shape, state):
    frames = {}
    for top_down in (False, True):
        planned, in_kernel, *_ = single_launches(gpu, shape, state, top_down)
        assert np.array_equal(planned, in_kernel), (shape, state, top_down, lsb_report(planned, in_kernel))
        frames[top_down] = planned
    assert np.array_equal(frames[True], frames[False][::-1]), (shape, state, "top_down is not the frame upside down")
    assert frames[False].std() > 1.0                                 # (a frame, not a constant)


@pytest.mark.parametrize("shape,state", [("192x100", "clamp"), ("130x55", UNDER_ONE_TEXEL)])
def test_planned_frame_within_one_lsb_of_the_oracle(gpu, shape, state):
    """The plan's frames against the oracle on the shapes with a partial last block: at the clamp over the small background, and with
    the lines' taps spread over three cells"""
    w, h, _ = shape_of(shape, state)
    planned, _, u, arrays, params = single_launches(gpu, shape, state, False)
    screen = O.render("visualizer", u, oracle_textures(arrays, params), w*2, h*2, threads=THREADS)
    want = O.resolve(screen, w, h, 2, threads=THREADS)
    d = np.abs(planned.astype(np.int32) - want.astype(np.int32))
    print(f"{shape}: {lsb_report(planned, want)}")
    assert d.max() <= 1, (shape, lsb_report(planned, want), np.argwhere(d > 1)[:5].tolist())
    assert_within_lsb(planned, want)


# ---- tape launches of three frames -----------------------------------------------------------------------------------------------------
FRAMES = 3


def clip_of(state):
    """(pcm, first tape slot, what the slots' volumes must be) of an audio state: the 1 s sweep driven into clipping reaches the clamp,
    zeros are silent"""
    from shaderflow_amd import synth
    sweep = synth.sweep_clip(1.0, 44100)
    if state == "silence":
        return np.zeros_like(sweep), 1, lambda v: bool((v == 0.0).all())
    return np.clip(4.0*sweep, -1.0, 1.0).astype(np.float32), 20, lambda v: bool((v > 0.62).all())


@pytest.mark.parametrize("state", sorted(STATES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_tape_launch_of_three_frames_same_bytes_with_and_without_the_plan(shape, state):
    from shaderflow_amd import synth
    from shaderflow_amd.tape import FrameTape
    from tests.test_gpu_tape_parity import prepared, scene_of
    w, h, bg_size = shape_of(shape, state)
    pcm, first, volumes_fit = clip_of(state)
    background = synth.background_image(bg_size[0], bg_size[1], seed=5)
    scene = prepared(scene_of("visualizer", pcm, background), w, h, 2, seconds=1.0)
    if STATES[state][1]:
        scene.camera.zoom.set(CAMERA["iCameraZoom"])
        scene.camera.position.set(np.array(CAMERA["iCameraPosition"]))
    tape = FrameTape(scene, batch=first + FRAMES).prepare(first + FRAMES)
    tape.bind_static_uniforms()
    N.check(N.lib().sfx_tape_reset(tape.handle))
    frame_bytes = w*h*3
    buffer = scene.context.alloc(frame_bytes*FRAMES)
    try:
        tape.build(0, first + FRAMES)
        volumes = tape.read(N.TAPE_UNIFORMS, FRAMES, first_slot=first)[:, 2]
        assert volumes_fit(volumes), (state, volumes.tolist())
        if state == UNDER_ONE_TEXEL:
            radii = [radius_in_texels(v, bg_size[1]) for v in volumes]
            assert all(0.9 <= r < 1.0 for r in radii), radii

        def launch(value, name):
            with switched(value):
                tape.render(FRAMES, buffer, first_slot=first)
                assert N.lib().sfx_last_kernel().decode() == name, N.lib().sfx_last_kernel()
            scene.context.synchronize()
            return scene.context.read(buffer, frame_bytes*FRAMES).reshape(FRAMES, h, w, 3).copy()
        frames = {}
        for top_down in (False, True):
            N.check(N.lib().sfx_ctx_output_top_down(scene.context.handle, int(top_down)))
            try:
                planned, in_kernel = launch(None, INSTANCE), launch("0", IN_KERNEL)
            finally:
                N.check(N.lib().sfx_ctx_output_top_down(scene.context.handle, 0))
            assert np.array_equal(planned, in_kernel), (shape, state, top_down, lsb_report(planned, in_kernel))
            frames[top_down] = planned
        assert not np.array_equal(frames[True], frames[False])      # (the switch reached the launch)
        assert frames[False].std() > 1.0
        if state != "silence":
            assert not np.array_equal(frames[False][0], frames[False][FRAMES - 1])     # (a table per frame)
    finally:
        scene.context.synchronize()
        scene.context.free(buffer)
        tape.release()
