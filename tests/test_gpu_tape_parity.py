"""
The path bench.py times — `FrameTape.build` + `sfx_render_tape`, 60 or 300 frames per launch — held to the contract stage by stage.
test_gpu_fullsize.py compares the tape's frames with the oracle running on the ORACLE's own audio tape: two stages at once, so it can
only ask for the edge-aware bound (a supersample on a bar's outline may change sides). Here the two stages are split:

  audio   the device tape of every frame of the benchmark's 60 s sweep (3 600 frames, 60 batches) against oracle_audio_tape within
          1e-5 relative, the loudness targets bit for bit; a 300-frame tape byte-equal to the 60-frame one (bank rotation, state hand-over)
  pixels  whole frames of every tape configuration bench.py times against oracle_tape_frame fed the DEVICE's own tape values of that
          frame — max <= 1 LSB on every value: C3 (60- and 300-frame launches, per-frame tables, the fixed blur bound of the tape
          launch), C2 (no SSAA: two passes), 1920x1080 2xSSAA, MusicBars and Waveform at 3840x2160 2xSSAA
  tier    the strip kernel's pixel tier (k_visualizer_classify) on flashes and spectra that put many tiles near its 0.4-LSB budget
  scroll  the per-frame states of a scrolling spectrogram texture, bit-exact against a numpy restatement of spectrogram.py:update
"""
import os
import time

import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import synth
from tests import replay as R
from tests.helpers import Gpu, gpu_bind_all, oracle_textures, smooth_spectrum, usable_cores, visualizer_inputs

pytestmark = pytest.mark.gpu
THREADS = usable_cores()
SECONDS, FPS, FRAMES = 60.0, 60.0, 3600
STATIC = dict(iDuration=SECONDS, iFramerate=FPS)                    # what the prepared scene pushes once (set_duration, fps)


def prepared(scene, w, h, ssaa, seconds=SECONDS):
    """A scene as `scene.main()` leaves it before the first frame (bench.py's build_scene)"""
    from shaderflow_amd.message import ShaderMessage
    scene.initialize()
    scene.exporting = scene.freewheel = scene.headless = True
    scene.realtime = False
    scene.fps, scene.subsample, scene.time = FPS, 2, 0.0
    scene.relay(ShaderMessage.Shader.Compile)
    scene.resize(width=w, height=h)
    for module in scene.modules:
        module.setup()
    scene.set_duration(seconds)
    scene.ssaa = ssaa
    return scene


def scene_of(kind, pcm, background):
    from examples.scenes import MusicBars, Visualizer, Waveform, make
    cls = {"visualizer": Visualizer, "bars": MusicBars, "waveform": Waveform}[kind]
    return make(cls, audio=(pcm, 44100), background=(background if kind == "visualizer" else None))


class TapeRun:
    """One pass of the export's tape over `frames` frames: every section of every frame, and the picked frames as rendered"""


def tape_run(kind, w, h, ssaa, pcm, background, batch, frames, picks=(), variants=({},)):
    """Build the tape batch by batch as the export does, read every frame's sections (sfx_tape_read), and render the batches that hold a
    picked frame in ONE launch each — once per `variants` entry (environment settings that choose another kernel instance)"""
    from shaderflow_amd import _native as N
    from shaderflow_amd.tape import FrameTape
    scene = prepared(scene_of(kind, pcm, background), w, h, ssaa)
    tape = FrameTape(scene, batch=batch).prepare(frames)
    tape.bind_static_uniforms()
    N.check(N.lib().sfx_tape_reset(tape.handle))
    sections = {"columns": N.TAPE_SPECTROGRAM, "targets": N.TAPE_TARGETS, "rows": N.TAPE_WAVEFORM, "uniforms": N.TAPE_UNIFORMS,
                "loudness": N.TAPE_LOUDNESS}
    run = TapeRun()
    run.tape = {name: [] for name in sections}
    run.frames = [{} for _ in variants]
    run.kernels = [set() for _ in variants]
    run.clock, run.dts = tape.clock.copy(), np.asarray(tape.dts)
    frame_bytes = w*h*3
    buffer = scene.context.alloc(frame_bytes*batch) if picks else None
    try:
        for first in range(0, frames, batch):
            count = min(batch, frames - first)
            tape.build(first, count)
            for name, what in sections.items():
                run.tape[name].append(tape.read(what, count))
            inside = [k for k in picks if first <= k < first + count]
            for v, variant in enumerate(variants if inside else ()):
                saved = {key: os.environ.get(key) for key in variant}
                os.environ.update(variant)
                try:
                    tape.render(count, buffer)
                    run.kernels[v].add(N.lib().sfx_last_kernel().decode())
                finally:
                    for key, value in saved.items():
                        if value is None:
                            os.environ.pop(key, None)
                        else:
                            os.environ[key] = value
                scene.context.synchronize()
                for k in inside:
                    run.frames[v][k] = scene.context.read(buffer + (k - first)*frame_bytes, frame_bytes).reshape(h, w, 3).copy()
    finally:
        scene.context.synchronize()
        if buffer is not None:
            scene.context.free(buffer)
        tape.release()
    run.tape = {name: np.concatenate(parts) for name, parts in run.tape.items()}
    return run


def device_values(run: TapeRun, k: int) -> dict:
    """Frame k's per-frame values as the device's tape holds them (FrameDyn: iTime, iTau, volume, integral, std, offset, iFrame), in the
    keys of R.oracle_tape_frame; iDeltatime is the host clock's (the fragments do not read it)"""
    u = run.tape["uniforms"][k]
    return dict(iTime=float(u[0]), iTau=float(u[1]), iAudioVolume=float(u[2]), iAudioVolumeIntegral=float(u[3]), iAudioSTD=float(u[4]),
                iFrame=int(u[6:7].view(np.int32)[0]), iDeltatime=float(run.dts[k]),
                iSpectrogram=run.tape["columns"][k], iWaveform=run.tape["rows"][k])


def histogram(got, want) -> np.ndarray:
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    return np.bincount(np.minimum(d.ravel(), 3), minlength=4)


def assert_within_one(got, want, where):
    counts = histogram(got, want)
    print(f"{where}: |d| histogram 0: {counts[0]}, 1: {counts[1]}, 2: {counts[2]}, >2: {counts[3]}")
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    assert counts[2:].sum() == 0, (where, counts.tolist(), np.argwhere(d > 1)[:6].tolist())


@pytest.fixture(scope="module")
def clip():
    pcm, background = synth.sweep_clip(SECONDS, 44100), synth.background_image(1920, 1080, seed=0)
    started = time.perf_counter()
    oracle = R.oracle_audio_tape(pcm, 44100, FPS, FRAMES, duration=SECONDS)
    print(f"oracle audio tape, {FRAMES} frames: {time.perf_counter() - started:.1f} s")
    return pcm, background, oracle, O.make_texture(np.flipud(background))


C3_PICKS = (0, 59, 60, 1500, 3599)                                  # dt = 0; the last and first frame of a batch; mid-clip; iTau near 1


@pytest.fixture(scope="module")
def c3(clip):
    """The benchmark's tape at C3 (3840x2160 2xSSAA) over the whole clip: in 60-frame batches (the picked frames rendered), and in
    300-frame batches as bench.py runs it (its first launch rendered: frame 299 lies at the far end of the 7.46 GB buffer)"""
    pcm, background, _, _ = clip
    started = time.perf_counter()
    small = tape_run("visualizer", 3840, 2160, 2, pcm, background, 60, FRAMES, C3_PICKS)
    big = tape_run("visualizer", 3840, 2160, 2, pcm, background, 300, FRAMES, (299,))
    print(f"device tapes of {FRAMES} frames, 60- and 300-frame batches, five launches: {time.perf_counter() - started:.1f} s")
    return small, big


def test_audio_tape_of_every_frame_of_the_benchmark_clip(c3, clip):
    """Every field of the device's tape, all 3 600 frames of the 60 s sweep (60 batches of 60), against the oracle's audio tape"""
    small, big = c3
    oracle = clip[2]
    t = small.tape
    peak = float(np.abs(oracle.columns).max())
    for name in ("targets", "columns"):                             # (the peak-relative floor of test_frame_tape_against_reference_pipeline)
        want = getattr(oracle, name)
        assert t[name].shape == want.shape
        bad = ~np.isclose(t[name], want, rtol=1e-5, atol=1e-9*peak)
        assert not bad.any(), (name, np.argwhere(bad)[:5].tolist(), float(np.abs(t[name] - want).max()))
    assert np.allclose(t["rows"], oracle.rows, rtol=1e-5, atol=1e-9), float(np.abs(t["rows"] - oracle.rows).max())
    # the loudness targets are numpy's bits on both sides (tests/loudness_ref.py has the order; the oracle is held to it on the CPU)
    assert np.array_equal(t["loudness"].astype(np.float64), oracle.loudness), np.argwhere(t["loudness"] != oracle.loudness)[:5].tolist()
    for column, want in ((2, oracle.volume), (3, oracle.integral), (4, oracle.std)):
        bad = ~np.isclose(t["uniforms"][:, column], want, rtol=1e-5, atol=1e-9)
        assert not bad.any(), (column, np.argwhere(bad)[:5].ravel().tolist())
    frames = t["uniforms"][:, 6].copy().view(np.int32)
    assert np.array_equal(frames, np.array([round(x*FPS) for x in oracle.times], np.int32))
    assert np.array_equal(t["uniforms"][:, 0], small.clock["iTime"]) and np.array_equal(t["uniforms"][:, 1], small.clock["iTau"])
    assert small.tape["uniforms"][-1, 1] > 0.99                      # (the clip's end: iTau near 1)
    # one launch of 300 frames builds the same tape: every section byte-equal (banks rotate, the recurrences hand over every 300 frames)
    for name in small.tape:
        assert big.tape[name].tobytes() == small.tape[name].tobytes(), name


@pytest.mark.timeout(600)
@pytest.mark.parametrize("k", [*C3_PICKS, 299])
def test_c3_tape_frame_within_one_lsb_of_the_oracle_on_the_device_tape(c3, clip, k):
    """Whole C3 frames of the tape launch (k_visualizer_strip<72, 12, 2, 9, ...>, grid.z = 60; frame 299 from the 300-frame launch)
    against the oracle fed the device's own tape values of that frame: `max <= 1` on every value"""
    small, big = c3
    run = big if k == 299 else small
    assert run.kernels[0] and all(name.startswith("k_visualizer_strip<72, 12, 2, 9, ") for name in run.kernels[0]), run.kernels
    started = time.perf_counter()
    want = R.oracle_tape_frame("visualizer", device_values(run, k), STATIC, 3840, 2160, 2, 2, background=clip[3], threads=THREADS)
    print(f"C3 oracle frame {k}: {time.perf_counter() - started:.1f} s on {THREADS} threads")
    assert_within_one(run.frames[0][k], want, f"C3 tape frame {k}{' (300-frame launch)' if run is big else ''}")


# the other tape configurations bench.py times: (kind, width, height, ssaa, frames, kernel instances as environment variants)
OTHER = {
    "c2": ("visualizer", 1920, 1080, 1, (1, 20, 39, 59, 60), ({},)),
    "1080p_2x": ("visualizer", 1920, 1080, 2, (59, 60), ({},)),
    "bars": ("bars", 3840, 2160, 2, (59, 60), ({}, {"SHADERFLOW_SEPARABLE_RUNS": "0"})),
    "waveform": ("waveform", 3840, 2160, 2, (59, 60), ({}, {"SHADERFLOW_SEPARABLE_RUNS": "0"})),
}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("config", list(OTHER))
def test_other_tape_configurations_within_one_lsb_of_the_oracle_on_the_device_tape(clip, config):
    """C2 (strip kernel into iScreen, then the resolve), the 2x instance for 1920x1080, and MusicBars / Waveform at 3840x2160 2xSSAA
    (k_separable_runs, and k_separable_fused with SHADERFLOW_SEPARABLE_RUNS=0) through the tape, two batches of 60: whole frames
    against the oracle on the device's tape values, `max <= 1` on every value"""
    kind, w, h, ssaa, picks, variants = OTHER[config]
    pcm, background, _, bg = clip
    run = tape_run(kind, w, h, ssaa, pcm, background, 60, picks[-1] + 1, picks, variants)
    print(f"{config}: kernels {run.kernels}")
    # MusicBars samples no waveform and Waveform no spectrogram (their tapes hold a one-point row / a private two-bin column)
    for k in picks:
        want = R.oracle_tape_frame({"bars": "bars", "waveform": "waveform"}.get(kind, "visualizer"), device_values(run, k), STATIC, w, h, ssaa, 2,
                                   background=(bg if kind == "visualizer" else None), waveform_smooth=(kind != "waveform"), threads=THREADS)
        for v in range(len(variants)):
            assert_within_one(run.frames[v][k], want, f"{config} frame {k} {sorted(run.kernels[v])}")
    expected = {"c2": ("k_visualizer_strip<66, 22, 1, 2, ",), "1080p_2x": ("k_visualizer_strip<120, 13, 2, 6, ",), "bars": ("k_separable_runs<bars>", "k_separable_fused<bars>"),
                "waveform": ("k_separable_runs<waveform>", "k_separable_fused<waveform>")}[config]
    for v, prefix in enumerate(expected):
        assert run.kernels[v] and all(name.startswith(prefix) for name in run.kernels[v]), (config, run.kernels)


def stepped_spectrum(bins: int = 115, seed: int = 0) -> np.ndarray:
    """Plateaus of 3-9 bins at heights from nothing to taller than the frame: tall bars whose neighbours differ by whole bar heights at
    every step, flat in between — tiles just outside a plateau's bars see the largest `drr` the classification allows for"""
    rng = np.random.default_rng(seed)
    column, b = np.zeros((bins, 2)), 0
    while b < bins:
        run = int(rng.integers(3, 10))
        column[b:b + run] = rng.choice([0.5, 40.0, 300.0, 1500.0, 6000.0], size=2)
        b += run
    return column.reshape(bins, 1, 2).astype(np.float32)


# (iAudioSTD, spectrum, seed): the flash c.flash = 5*iAudioSTD from off to 2.5x the largest the clip reaches (clip_max); tall smooth
# bars, tall stepped bars, and a low column whose ring sits just outside the disc
TIER_CASES = {"no_flash_tall": (0.0, "smooth", 91), "clip_max_flash": ("clip_max", "smooth", 92),
              "beyond_clip_stepped": ("2.5 clip_max", "stepped", 93), "clip_max_low": ("clip_max", "low", 94)}


@pytest.fixture()
def gpu():
    g = Gpu()
    yield g
    g.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("case", list(TIER_CASES))
def test_c3_pixel_tier_within_one_lsb_of_the_oracle(gpu, clip, case):
    """Whole C3 frames with the pixel tier on (the default) against the oracle, `max <= 1` on every value, on inputs that push many tiles
    near the tier's 0.4-LSB budget; the tier must serve a substantial share of the waves (so the case cannot pass by not running it)"""
    std, kind, seed = TIER_CASES[case]
    clip_max = float(clip[2].std.max())
    std = {"clip_max": clip_max, "2.5 clip_max": 2.5*clip_max}.get(std, std)
    w, h, ssaa = 3840, 2160, 2
    u, arrays, params = visualizer_inputs(w, h, seed=seed, volume=0.8, std=std, bg_size=(1920, 1080))
    arrays["background"] = np.ascontiguousarray(np.flipud(synth.background_image(1920, 1080)))
    arrays["iSpectrogram"] = {"smooth": lambda: smooth_spectrum(seed=seed), "stepped": lambda: stepped_spectrum(seed=seed),
                              "low": lambda: smooth_spectrum(seed=seed)*np.float32(0.02)}[kind]()
    u.iSSAA = float(ssaa)
    prog, _ = gpu.program("visualizer")
    gpu.set_uniforms(prog, u)
    gpu_bind_all(gpu, prog, arrays, params)
    gpu.ctx.tile_misses()
    got = gpu.render_resolve(prog, w, h, ssaa, 2)
    per_sample = gpu.ctx.tile_misses()
    assert gpu.lib.sfx_last_kernel().decode() == "k_visualizer_strip<72, 12, 2, 9, 6, 4, false>", gpu.lib.sfx_last_kernel()
    waves = (w*ssaa//64)*(h*ssaa//9)
    print(f"{case}: iAudioSTD {std:.3f}, {per_sample} of {waves} waves per sample ({100*(1 - per_sample/waves):.1f} % by the tier)")
    screen = O.render("visualizer", u, oracle_textures(arrays, params), w*ssaa, h*ssaa, threads=THREADS)
    assert_within_one(got, O.resolve(screen, w, h, 2, threads=THREADS), f"pixel tier, {case}")
    assert 0 < per_sample < 0.75*waves, (per_sample, waves)


@pytest.mark.parametrize("seconds,batch,frames", [(0.12, 60, 150), (1.5, 60, 200), (0.5, 45, 100)])
def test_scrolling_spectrogram_states_bit_exact(seconds, batch, frames):
    """ShaderSpectrogram(length=seconds) through the tape: the texture state every frame of a batch sees (TAPE_SCROLL) equals
    spectrogram.py:update restated in numpy — column (k + 1) % width takes frame k's smoothed column, zeros before any frame wrote
    it — for widths below, above and not dividing the batch, over several batches (the ring wraps); after sfx_tape_reset the texture
    starts empty again"""
    from shaderflow_amd import ShaderScene
    from shaderflow_amd import _native as N
    from shaderflow_amd.audio import ShaderAudio
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    from shaderflow_amd.piano import PianoNote
    from shaderflow_amd.tape import FrameTape
    from tests.helpers import SCROLL_FRAGMENT
    pcm = synth.sweep_clip(frames/FPS + 0.5, 44100)

    class Scroller(ShaderScene):
        def build(self):
            super().build()
            self.audio = ShaderAudio(scene=self, name="iAudio")
            self.audio.load(samples=pcm, samplerate=44100)
            self.spectrogram = ShaderSpectrogram(scene=self, audio=self.audio, length=seconds)
            self.spectrogram.from_notes(start=PianoNote.from_frequency(20), end=PianoNote.from_frequency(14000), piano=True)
            self.shader.fragment = SCROLL_FRAGMENT

    scene = prepared(Scroller(), 320, 180, 1, seconds=frames/FPS)
    width = scene.spectrogram.length_samples
    assert width == int(seconds*FPS) and width > 1
    tape = FrameTape(scene, batch=batch).prepare(frames)
    try:
        for attempt in range(2):                                    # the second pass after sfx_tape_reset: the same states
            N.check(N.lib().sfx_tape_reset(tape.handle))
            state = None
            for first in range(0, frames if attempt == 0 else batch, batch):
                count = min(batch, frames - first)
                tape.build(first, count)
                columns, got = tape.read(N.TAPE_SPECTROGRAM, count), tape.read(N.TAPE_SCROLL, count)
                if state is None:
                    state = np.zeros(got.shape[1:], np.float32)     # (bins, width, channels): empty before the first write
                for f in range(count):
                    state[:, (first + f + 1) % width, :] = columns[f]
                    assert np.array_equal(got[f], state), (attempt, first + f, np.argwhere(got[f] != state)[:4].tolist())
                assert np.abs(columns).max() > 0                    # (the clip is not silent: a state of zeros would not be checked)
    finally:
        tape.release()
