"""
The strip kernel's diagonal walk (VisualizerStrip::run, "the four diagonal directions"): in the float32-cell instances one running pair for
both y sides of a walk step, a half fold where a side enters the next row of cells, a full fold of both sides where one jumps further; in
the float16-cell instances an accumulation per side, with the table's other format. Whole small frames against the
oracle within 1 LSB, at the smallest shapes at which each of those paths — and the per-frame table behind them (k_visualizer_axes'
ysteps) — can go wrong; every frame rendered twice (the kernel is deterministic). Which instance the dispatcher picks is its own business:
only the family is asserted, the instance's name is printed with a failure.
"""
import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import _native as N
from tests.helpers import Gpu, gpu_bind_all, lsb_report, oracle_textures, usable_cores, visualizer_inputs
from tests.test_gpu_pixels import assert_within_lsb

pytestmark = pytest.mark.gpu
THREADS = usable_cores()


@pytest.fixture()
def gpu():
    g = Gpu()
    yield g
    g.close()


def last_kernel(gpu) -> str:
    return gpu.lib.sfx_last_kernel().decode()


def render_case(gpu, w, h, ssaa, bg_size, volume, camera=None, repeat=(True, True), top_down=False, seed=41):
    """One frame on the device (twice) and on the oracle: (got, want, kernel)"""
    u, arrays, params = visualizer_inputs(w, h, seed=seed, volume=volume, bg_size=bg_size)
    params["background"] = ("linear", repeat[0], repeat[1])
    for key, value in (camera or {}).items():
        cur = getattr(u, key)
        if hasattr(cur, "__len__"):
            for i, v in enumerate(value):
                cur[i] = v
        else:
            setattr(u, key, value)
    u.iSSAA = float(ssaa)
    screen = O.render("visualizer", u, oracle_textures(arrays, params), w*ssaa, h*ssaa, threads=THREADS)
    want = screen if ssaa == 1 else O.resolve(screen, w, h, 2, threads=THREADS)
    prog, _ = gpu.program("visualizer")
    gpu.set_uniforms(prog, u)
    gpu_bind_all(gpu, prog, arrays, params)

    def once():
        return gpu.render(prog, w, h) if ssaa == 1 else gpu.render_resolve(prog, w, h, ssaa, 2)
    N.check(gpu.lib.sfx_ctx_output_top_down(gpu.ctx.handle, int(top_down)))
    try:
        got = once()
        kernel = last_kernel(gpu)
        again = once()
    finally:
        N.check(gpu.lib.sfx_ctx_output_top_down(gpu.ctx.handle, 0))
    assert np.array_equal(got, again), (kernel, "two launches of the same frame differ", lsb_report(got, again))
    if top_down:
        want = want[::-1]
    return got, want, kernel


def check(gpu, *args, **kwargs):
    got, want, kernel = render_case(gpu, *args, **kwargs)
    assert kernel.startswith("k_visualizer_strip<"), kernel
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{kernel}: {lsb_report(got, want)}")
    assert d.max() <= 1, (kernel, lsb_report(got, want), np.argwhere(d > 1)[:5].tolist())
    assert_within_lsb(got, want)


CAMERAS = {"zoom 0.6": dict(iCameraZoom=0.6, iCameraPosition=(0.11, -0.07, 0.0)), "zoom 1.8": dict(iCameraZoom=1.8, iCameraPosition=(0.11, -0.07, 0.0))}


def test_strips_with_no_crossing_or_exactly_one(gpu):
    """0.075 texel per sample: most strips stay in one row of cells for a whole walk step (the running pair is never touched after the
    first row), some cross once"""
    check(gpu, 640, 360, 2, (96, 54), 0.9)


def test_radius_zero_both_sides_in_the_same_cell_row(gpu):
    """A silent frame: the displacement is 0, y+ and y- are the same coordinate and cross at the same row gap (y* of both sides equal)"""
    check(gpu, 600, 362, 2, (384, 216), 0.0)


def test_largest_radius_two_or_three_crossings_per_side(gpu):
    """The radius at its clamp (0.3): the sides lie furthest apart, each crosses two or three times per strip"""
    check(gpu, 600, 362, 2, (384, 216), 2.5)


@pytest.mark.parametrize("w,h,bg_size", [(200, 41, (32, 18)), (520, 365, (384, 216))])
def test_last_row_group_of_one_row_and_partial_columns(gpu, w, h, bg_size):
    """2h = 10 mod 18: the frame's last wave of nine-row strips holds ONE row (the first row's fold and nothing else; the rows behind it
    read the table past the frame's end), and the width is no multiple of a block's 128 pixels. (The 82 sample rows of the small frame
    over a 216-row background are 2.2 texels apart — no strip instance's tile holds a block's window then, the dispatcher takes the
    generic kernel — so the small frame gets a background at the strip kernels' density: 0.19 texel per sample.)"""
    check(gpu, w, h, 2, bg_size, 1.3)


def test_dense_float16_instance(gpu):
    """About 0.45 texel per sample: a float16-cell instance — these keep an accumulation per side, and k_visualizer_axes writes the
    FRACTIONS into their walk-step table where the float32-cell instances get y* (one builder, two formats, chosen by the cell size)"""
    check(gpu, 520, 363, 2, (640, 360), 0.9)


def test_four_times_ssaa(gpu):
    check(gpu, 160, 90, 4, (256, 144), 0.9)


def test_no_ssaa_nearly_a_texel_per_sample(gpu):
    """No SSAA into an RGBA8 iScreen (float16 cells, the table's fractions), strips of two rows at the largest distance between samples a
    strip instance takes: 0.9 texel, a side enters the next row of cells at nearly every row. (64 sample columns must fit a tile 66 cells
    wide, so no strip instance sees samples MORE than a texel apart — over a 216-row background this frame goes to the generic kernel;
    the shared form's full fold of both sides for a side that skips a row of cells is the net under that bound, not a path a frame can
    be aimed at.)"""
    check(gpu, 300, 170, 1, (320, 180), 0.9)


@pytest.mark.parametrize("camera", sorted(CAMERAS))
def test_zoomed_and_panned_camera(gpu, camera):
    """Zoomed out the samples lie further apart (a crossing at nearly every second row, another instance), zoomed in closer together; the
    pan moves the window off the centre"""
    check(gpu, 600, 362, 2, (384, 216), 0.9, camera=CAMERAS[camera])


def test_top_down_rows(gpu):
    check(gpu, 600, 362, 2, (384, 216), 0.9, top_down=True)


def test_repeat_wrap_over_the_textures_edge(gpu):
    """A small repeating background under a camera that sees past its edges on every side: the staged window wraps in both directions and
    the walk's rows of cells run across the seam"""
    check(gpu, 256, 144, 2, (64, 36), 0.9, camera=dict(iCameraZoom=0.7, iCameraPosition=(0.3, 0.2, 0.0)))


def test_tape_launch_of_eight_frames_equals_single_launches():
    """The walk-step table is per frame ([frame][row][10]): eight frames of a tape whose blur radius differs from frame to frame in ONE
    launch, against the same eight tape slots rendered by one launch each — byte for byte (the same kernel on the same values; a wrong
    frame stride of the table, or of the row entries the kernel takes the rows' coordinates from, shows here)"""
    from shaderflow_amd import synth
    from shaderflow_amd.tape import FrameTape
    from tests.test_gpu_tape_parity import prepared, scene_of
    w, h, ssaa, frames, first = 384, 216, 2, 8, 1               # (the clip's first two frames are both silent: slots 1..8)
    pcm, background = synth.sweep_clip(1.0, 44100), synth.background_image(192, 108, seed=3)    # 0.21 texel per sample: the float32-cell instance, the shared form
    scene = prepared(scene_of("visualizer", pcm, background), w, h, ssaa, seconds=1.0)
    tape = FrameTape(scene, batch=first + frames).prepare(first + frames)
    tape.bind_static_uniforms()
    N.check(N.lib().sfx_tape_reset(tape.handle))
    frame_bytes = w*h*3
    together, single = scene.context.alloc(frame_bytes*frames), scene.context.alloc(frame_bytes)
    try:
        tape.build(0, first + frames)
        volumes = tape.read(N.TAPE_UNIFORMS, frames, first_slot=first)[:, 2]
        assert len(set(volumes.tolist())) == frames and 0.0 < volumes.max() < 0.61, volumes     # 0.01*volume^2.5 below its clamp: a radius per frame
        tape.render(frames, together, first_slot=first)
        kernel = N.lib().sfx_last_kernel().decode()
        assert kernel.startswith("k_visualizer_strip<"), kernel
        scene.context.synchronize()
        whole = scene.context.read(together, frame_bytes*frames).reshape(frames, h, w, 3).copy()
        for k in range(frames):
            tape.render(1, single, first_slot=first + k)
            assert N.lib().sfx_last_kernel().decode() == kernel
            scene.context.synchronize()
            alone = scene.context.read(single, frame_bytes).reshape(h, w, 3)
            assert np.array_equal(whole[k], alone), (kernel, k, lsb_report(whole[k], alone))
        assert not np.array_equal(whole[0], whole[frames - 1])
    finally:
        scene.context.synchronize()
        scene.context.free(together)
        scene.context.free(single)
        tape.release()
