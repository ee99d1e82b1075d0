"""
Scene-level parity on the GPU: the python API (ShaderScene/ShaderModule/…) drives the C-ABI and the frames are
compared with the oracle run on the oracle's own audio tape — the whole path of SURVEY.md §3.2, end to end.
End-to-end tolerance: 1 LSB on every value (tape values within 1e-5 relative feed the fragments, so a pixel sitting on a
branch boundary could flip in principle; none does in these scenes). Stage-wise tests (test_gpu_audio / test_gpu_pixels)
hold each stage to its strict bound; tests/test_gpu_fullsize.py has the whole frames at the benchmark's sizes.
"""
import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import synth
from tests.helpers import lsb_report

pytestmark = pytest.mark.gpu


def clip(seconds=0.5, samplerate=44100, seed=0):
    rng = np.random.default_rng(seed)
    pcm = synth.sweep_clip(seconds, samplerate)
    pcm[int(0.3*len(pcm)):int(0.5*len(pcm))] += (0.25*rng.standard_normal((int(0.5*len(pcm)) - int(0.3*len(pcm)), 2))).astype(np.float32)
    return np.clip(pcm, -1, 1).astype(np.float32), samplerate


def frames_of(raw: bytes, w, h):
    return np.frombuffer(raw, np.uint8).reshape(-1, h, w, 3)


def oracle_visualizer_frames(pcm, samplerate, background, w, h, ssaa, subsample, fps, frames, runtime):
    """The reference's frame loop restated on the oracle: audio tape (sfo_audio.c) → fragments (sfo_pixel.c)"""
    planar = np.ascontiguousarray(pcm.T)
    times, dts, rdts = O.clock(fps, frames)
    _, tell = O.reader(rdts, samplerate, 2, planar.shape[1])
    fmin, fmax, bins = O.from_notes(O.lib().sfo_note_of_frequency(20.0, 440.0), O.lib().sfo_note_of_frequency(14000.0, 440.0), True)
    indptr, indices, data = O.filterbank(0, 0, fmin, fmax, bins, 12, samplerate)
    volume, std, spec = O.DynF64(0.0, 2, 1, 0, integrate=True), O.DynF64(0.0, 10, 1, 0), O.DynF32(2*bins, 4, 1, 0)
    bg = O.make_texture(np.flipud(background), "linear", True, True)             # from_numpy flips (texture.py:327-335)
    out = []
    for k in range(frames):
        vt, st = O.volume_std(planar, int(tell[k]), int(0.1*samplerate))
        volume.step(vt, abs(dts[k])); std.step(st, abs(dts[k]))
        row = O.waveform_row(planar, int(tell[k]), max(1, int(3*samplerate/180)), 180)
        target = O.csr_dot(indptr, indices, data, O.fft_power(planar, int(tell[k])))
        column = spec.step(target.ravel(), abs(dts[k])).copy()
        u = O.default_uniforms(w, h, iTime=times[k], iTau=(times[k]/runtime) % 1.0, iDuration=runtime, iDeltatime=dts[k],
                               iSSAA=float(ssaa), iFramerate=fps, iFrame=round(times[k]*fps), iSubsample=subsample,
                               iAudioVolume=volume.value.value, iAudioVolumeIntegral=volume.integral.value, iAudioSTD=std.value.value,
                               iSpectrogramLength=1, iSpectrogramBins=bins, iWaveformLength=180)
        tex = {"background": bg,
               "iSpectrogram": O.make_texture(column.reshape(bins, 1, 2), "nearest", True, False),
               "iWaveform": O.make_texture(row.reshape(1, 180, 2), "linear", False, False)}
        screen = O.render("visualizer", u, tex, w*ssaa, h*ssaa, threads=8)
        out.append(O.resolve(screen, w, h, subsample, threads=8))
    return np.stack(out)


def mostly_within_one_lsb(got, want, fraction=1.0):
    """Every value within 1 LSB — the north star's bound (round 2 accepted 0.1 % beyond it; the histogram of these scenes,
    profiles/r02_parity_histogram.txt, has no such value)"""
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and (d <= 1).mean() >= fraction, lsb_report(got, want)


def test_basic_scene_256(tmp_path):
    """BASELINE config 1: examples/basic default scene, 256x256 (1 s; here 6 frames), raw rgb24 output"""
    from examples.scenes import Basic
    scene = Basic()
    raw = scene.main(width=256, height=256, fps=60, time=0.1, output=bytes, batch=False)
    got = frames_of(raw, 256, 256)
    assert got.shape[0] == 6
    times, _, _ = O.clock(60.0, 6)
    for k in (0, 5):
        u = O.default_uniforms(256, 256, iTime=times[k], iTau=(times[k]/0.1) % 1.0, iDuration=0.1)
        want = O.resolve(O.render("default", u, {}, 256, 256, threads=8), 256, 256, 2)       # ssaa=1, subsample=2: 3x3 tent
        assert np.array_equal(got[k], want), lsb_report(got[k], want)
    path = Basic().main(width=64, height=64, fps=30, time=0.1, output=tmp_path/"basic.rgb")
    assert path.stat().st_size == 3*64*64*3


@pytest.mark.parametrize("ssaa,subsample", [(2, 2), (1, 2)])
def test_visualizer_frame_loop_and_tape_match_oracle(ssaa, subsample):
    """Visualizer scene: python frame loop (batch=False) and device frame tape (batch=True) vs the oracle"""
    from examples.scenes import Visualizer, make
    w, h, fps, seconds = 128, 72, 60.0, 0.2
    pcm, sr = clip(0.5)
    background = synth.background_image(160, 90, seed=1)
    frames = round(seconds*fps)
    want = oracle_visualizer_frames(pcm, sr, background, w, h, ssaa, subsample, fps, frames, seconds)

    loop = make(Visualizer, audio=(pcm, sr), background=background)
    raw = loop.main(width=w, height=h, fps=fps, ssaa=ssaa, subsample=subsample, time=seconds, output=bytes, batch=False)
    got_loop = frames_of(raw, w, h)
    assert got_loop.shape == want.shape
    mostly_within_one_lsb(got_loop, want)

    # the tape renders (2, 2) through the fused kernel and (1, 2) in two batched passes
    tape = make(Visualizer, audio=(pcm, sr), background=background)
    raw = tape.main(width=w, height=h, fps=fps, ssaa=ssaa, subsample=subsample, time=seconds, output=bytes, batch=None)
    got_tape = frames_of(raw, w, h)
    mostly_within_one_lsb(got_tape, want)
    mostly_within_one_lsb(got_tape, got_loop)


def test_tape_is_chosen_only_for_stock_scenes():
    from examples.scenes import Dynamics, Visualizer, make
    from shaderflow_amd.tape import FrameTape
    pcm, sr = clip(0.3)
    vis = make(Visualizer, audio=(pcm, sr), background=synth.background_image(64, 36))
    vis.initialize(); vis._ssaa = 2.0
    assert FrameTape.applicable(vis)
    vis._ssaa = 1.5                                               # fractional SSAA: two batched passes
    assert FrameTape.applicable(vis)
    dyn = Dynamics()
    dyn.initialize()
    assert not FrameTape.applicable(dyn)                          # python update() every frame


def test_dynamics_and_multishader_scenes_run():
    from examples.scenes import Dynamics, MultiShader
    raw = Dynamics().main(width=96, height=54, fps=30, time=0.2, output=bytes)
    assert frames_of(raw, 96, 54).shape[0] == 6 and frames_of(raw, 96, 54).std() > 1
    raw = MultiShader().main(width=64, height=36, fps=30, time=0.1, ssaa=2, output=bytes)
    img = frames_of(raw, 64, 36)[0]
    x = (np.arange(64) + 0.5)/64
    stuv = ((2*x - 1)*(64/36) + 1)/2
    assert np.abs(img[:, :, 0].astype(int) - np.rint(np.clip(stuv, 0, 1)*255)[None, :]).max() <= 1      # demo.py:74-89 closed form
    assert np.abs(img[:, :, 1].astype(int) - np.rint(np.clip(1 - stuv, 0, 1)*255)[None, :]).max() <= 1


def test_musicbars_and_waveform_scenes_run():
    from examples.scenes import MusicBars, Waveform, make
    pcm, sr = clip(0.3)
    raw = make(MusicBars, audio=(pcm, sr)).main(width=128, height=64, fps=60, time=0.15, output=bytes)
    bars = frames_of(raw, 128, 64)
    assert bars.shape[0] == 9 and bars[-1].max() == 255
    raw = make(Waveform, audio=(pcm, sr)).main(width=128, height=64, fps=60, time=0.15, output=bytes)
    assert frames_of(raw, 128, 64)[-1].max() == 255


def test_screenshot_and_texture_api():
    from examples.scenes import Basic
    from shaderflow_amd.texture import ShaderTexture
    scene = Basic()
    scene.main(width=64, height=36, fps=30, time=0.04, freewheel=True)
    shot = scene.screenshot()
    assert shot.shape == (36, 64, 3) and shot.dtype == np.uint8 and shot.std() > 0
    tex = ShaderTexture(scene=scene, name="probe")
    data = np.arange(4*3*2, dtype=np.float32).reshape(4, 3, 2)
    tex.from_numpy(data)
    assert tex.size == (3, 4) and tex.components == 2 and not tex.is_empty()
    assert np.array_equal(tex.texture.read(), np.flipud(data))
    with pytest.raises(Exception, match="too large"):
        ShaderTexture(scene=scene, name="huge", width=70000, height=8)


FAKE_FFMPEG = """#!/usr/bin/env python3
# stands in for the encoder in the hand-off test: records argv, copies the rawvideo stdin to the output path
import json, sys
argv = sys.argv[1:]
out = [a for a in argv if a.endswith(".mp4")][-1]
open(out + ".argv.json", "w").write(json.dumps(argv))
with open(out, "wb") as f:
    while chunk := sys.stdin.buffer.read(1 << 20):
        f.write(chunk)
"""


@pytest.mark.parametrize("batch", [None, False])
def test_encoder_handoff_top_down_rows_and_command(tmp_path, monkeypatch, batch):
    """with an ffmpeg process as the sink the frames arrive top-down (flipped while written on the device),
    the command is the reference's (exporting.py:91-120) minus `vflip`, and ShaderAudio.ffhook adds the audio track"""
    import json
    import os
    from examples.scenes import Visualizer, make
    from shaderflow_amd.audio.reader import write_wav_f32
    bindir = tmp_path/"bin"
    bindir.mkdir()
    (bindir/"ffmpeg").write_text(FAKE_FFMPEG)
    (bindir/"ffmpeg").chmod(0o755)
    monkeypatch.setenv("PATH", f"{bindir}{os.pathsep}{os.environ['PATH']}")
    pcm, sr = clip(0.3)
    wav = tmp_path/"clip.wav"
    write_wav_f32(wav, pcm, sr)
    background = synth.background_image(96, 54, seed=3)
    w, h, fps, seconds = 96, 54, 30.0, 0.2

    reference_stream = make(Visualizer, audio=wav, background=background).main(
        width=w, height=h, fps=fps, ssaa=2, time=seconds, output=bytes, batch=batch)          # rows bottom-up, as the reference pipes them
    want = frames_of(reference_stream, w, h)

    scene = make(Visualizer, audio=wav, background=background)
    scene.ffmpeg.h264(crf=18, preset="fast")
    out = scene.main(width=w, height=h, fps=fps, ssaa=2, time=seconds, output=tmp_path/"video.mp4", batch=batch)
    assert out == tmp_path/"video.mp4"
    got = frames_of(out.read_bytes(), w, h)
    assert got.shape == want.shape == (6, h, w, 3)
    assert np.array_equal(got, want[:, ::-1]), "frames handed to the encoder must be the bottom-up frames with rows reversed"

    argv = json.loads((tmp_path/"video.mp4.argv.json").read_text())
    assert argv == ["-hide_banner", "-loglevel", "error", "-f", "rawvideo", "-s", f"{w}x{h}", "-pix_fmt", "rgb24", "-r", "30.0", "-i", "-",
                    "-i", str(wav), "-t", "0.2", "-shortest", "-c:v", "libx264", "-movflags", "+faststart", "-preset", "fast", "-crf", "18",
                    "-vf", f"scale={w}x{h}:flags=lanczos", "-pix_fmt", "yuv420p", str(tmp_path/"video.mp4"), "-y"]

    # the next export of the same context is bottom-up again (the switch is reset in finish())
    again = make(Visualizer, audio=wav, background=background).main(width=w, height=h, fps=fps, ssaa=2, time=seconds, output=bytes, batch=batch)
    assert np.array_equal(frames_of(again, w, h), want)
    # raw sinks can ask for top-down rows explicitly
    flipped = make(Visualizer, audio=wav, background=background).main(width=w, height=h, fps=fps, ssaa=2, time=seconds, output=bytes,
                                                                        batch=batch, top_down=True)
    assert np.array_equal(frames_of(flipped, w, h), want[:, ::-1])


@pytest.mark.parametrize("name,ssaa", [("Basic", 1), ("Basic", 2), ("ShaderToy", 2), ("Mandelbrot", 1), ("RayMarch", 2), ("Plasma", 2), ("Bloom", 2), ("Bloom", 1)])
def test_clock_tape_equals_frame_loop(name, ssaa):
    """Scenes without audio modules batch through a clock-only tape (iTime/iTau/iFrame per frame on the device):
    the same kernels with the same uniform values, so the frames are identical to the python frame loop's"""
    import examples.scenes as scenes
    from shaderflow_amd.tape import FrameTape
    cls = getattr(scenes, name)
    probe = cls()
    probe.initialize()
    assert FrameTape.applicable(probe)
    kw = dict(width=96, height=54, fps=60, time=70/60, ssaa=ssaa, output=bytes)              # 70 frames: two batches of the tape
    loop = frames_of(cls().main(batch=False, **kw), 96, 54)
    tape = frames_of(cls().main(batch=None, **kw), 96, 54)
    assert loop.shape == tape.shape == (70, 54, 96, 3)
    assert np.array_equal(loop, tape), lsb_report(tape, loop)
    assert not np.array_equal(tape[0], tape[-1]) or name in ("Mandelbrot", "RayMarch")       # time-dependent scenes move


@pytest.mark.parametrize("ssaa", [1, 2, 4])
def test_bloom_scene_with_and_without_the_lds_tile(ssaa, monkeypatch):
    """examples.scenes.Bloom through scene.main (translate, compile, bind, tape): its glow loop makes the translator ask for the LDS
    tile; with SHADERFLOW_JIT_TILE=0 the same text compiles without it — the exported frames are the same bytes"""
    from examples.scenes import Bloom
    from shaderflow_amd import glsl2hip
    assert glsl2hip.translate(Bloom.FRAGMENT, [("sampler2D", "background")]).tiled_sampler == "background"
    kw = dict(width=200, height=112, fps=30, time=12/30, ssaa=ssaa, output=bytes)
    tiled = frames_of(Bloom().main(**kw), 200, 112)
    monkeypatch.setenv("SHADERFLOW_JIT_TILE", "0")
    assert glsl2hip.translate(Bloom.FRAGMENT, [("sampler2D", "background")]).tiled_sampler is None
    plain = frames_of(Bloom().main(**kw), 200, 112)
    assert tiled.shape == (12, 112, 200, 3) and np.array_equal(tiled, plain), lsb_report(tiled, plain)
    assert tiled.std() > 10 and not np.array_equal(tiled[0], tiled[-1])


@pytest.mark.parametrize("ssaa", [1, 2])
def test_waveform_scene_tape_equals_frame_loop(ssaa):
    """demo.py's Waveform scene (audio + waveform, no spectrogram module): the tape carries a private, detached spectrogram plan so
    that the scene still takes the batched path — same frames as the python frame loop, and the scene's module list, pipeline and
    fragment are untouched by it"""
    from examples.scenes import Waveform, make
    from shaderflow_amd.tape import FrameTape
    pcm, sr = clip(1.3)
    probe = make(Waveform, audio=(pcm, sr))
    probe.initialize()
    assert FrameTape.applicable(probe)
    kw = dict(width=160, height=90, fps=60, time=70/60, ssaa=ssaa, output=bytes)              # 70 frames: two batches of the tape
    loop_scene, tape_scene = make(Waveform, audio=(pcm, sr)), make(Waveform, audio=(pcm, sr))
    loop = frames_of(loop_scene.main(batch=False, **kw), 160, 90)
    tape = frames_of(tape_scene.main(batch=None, **kw), 160, 90)
    assert not any(getattr(m, "name", "") == "iTapePrivateSpectrogram" for m in tape_scene.modules)
    assert [type(m).__name__ for m in tape_scene.modules] == [type(m).__name__ for m in loop_scene.modules]
    assert loop.shape == tape.shape == (70, 90, 160, 3)
    assert np.abs(loop.astype(int) - tape.astype(int)).max() <= 1, lsb_report(tape, loop)
    assert not np.array_equal(tape[5], tape[40])


@pytest.mark.parametrize("batch", [1, 2, 3, 7])
def test_tape_banks_with_small_batches(batch, monkeypatch):
    """The tape's two banks and streams (capi_audio.hip Tape): with batches of a few frames the builds run far ahead of the renders and
    the banks alternate dozens of times — the frames must be the ones a single batch gives, for an audio scene with both passes
    (no SSAA: fragment into iScreen, then final.glsl) and for the fused path; tools/stress_tape_banks.py is the long version"""
    from examples.scenes import MusicBars, Visualizer, make
    from shaderflow_amd import synth
    from shaderflow_amd.tape import FrameTape
    frames = 45
    pcm, background = synth.sweep_clip(frames/60.0, 44100), synth.background_image(320, 180, seed=0)
    for cls, ssaa in ((MusicBars, 2), (Visualizer, 1), (Visualizer, 2)):
        kwargs = dict(audio=(pcm, 44100), **({"background": background} if cls is Visualizer else {}))
        kw = dict(width=192, height=108, fps=60.0, time=frames/60.0, ssaa=ssaa, output=bytes, batch=True)
        whole = frames_of(make(cls, **kwargs).main(**kw), 192, 108)
        monkeypatch.setattr(FrameTape, "BATCH", batch)
        small = frames_of(make(cls, **kwargs).main(**kw), 192, 108)
        monkeypatch.undo()
        assert np.array_equal(small, whole), (cls.__name__, ssaa, lsb_report(small, whole))


def test_piano_module_writes_its_textures(tmp_path):
    """ShaderPiano inside a scene: textures of the reference's shapes, written every frame, uniforms in the pipeline; a MIDI
    file round trip feeds it (the texture CONTENTS are pinned on CPU, tests/test_host_piano.py)"""
    from examples.scenes import Basic
    from shaderflow_amd.piano import PianoNote, ShaderPiano
    from shaderflow_amd.piano.midi import write_midi

    score = [PianoNote(note=60 + k % 12, start=0.05*k, end=0.05*k + 0.3, channel=k % 3, velocity=40 + 5*k) for k in range(16)]
    midi = write_midi(tmp_path/"score.mid", score)

    class PianoScene(Basic):
        def build(self):
            self.piano = ShaderPiano(scene=self)
            self.piano.load_midi(midi)

    scene = PianoScene()
    raw = scene.main(width=64, height=36, fps=30, time=0.5, output=bytes)
    assert frames_of(raw, 64, 36).shape[0] == 15
    piano = scene.piano
    assert len(list(piano.notes)) == 16 and piano.global_minimum_note == 60 and piano.global_maximum_note == 71
    assert piano.keys_texture.size == (128, 1) and piano.roll_texture.size == (256, 128) and piano.roll_texture.components == 4
    keys = piano.keys_texture.texture.read()[0, :, 0]
    assert np.array_equal(keys, piano.key_press_dynamics.value.astype(np.float32)) and keys[60:72].max() > 0
    roll = piano.roll_texture.texture.read()                        # (128 notes, 256 slots, 4), as written
    assert roll.shape == (128, 256, 4) and roll[60:72, 0, 1].max() > 0 and not roll[:60].any()
    channels = piano.channel_texture.texture.read()[0, :, 0]
    assert channels.min() == -1 and set(np.unique(channels[60:72])) <= {-1.0, 0.0, 1.0, 2.0}
    names = {u.name for u in scene.shader.full_pipeline()}
    assert {"iPianoDynamic", "iPianoRollTime", "iPianoKeys0x0", "iPianoRoll0x0", "iPianoChan0x0", "iPianoTempo0x0"} <= names


def test_scripted_camera_motion_matches_oracle():
    """A scene that drives the camera from update() (move, zoom, rotate2d, projection): every frame equals the oracle rendered
    with the uniforms the pipeline emitted for that frame (camera.py:196-235 → camera.glsl)"""
    from examples.scenes import Basic
    from shaderflow_amd.camera import CameraProjection
    from shaderflow_amd.module import ShaderModule

    snapshots = []

    class Snapshot(ShaderModule):
        def update(self):
            snapshots.append({v.name: np.array(v.value, dtype=np.float64).copy() for v in self.scene.shader.full_pipeline() if v.type != "sampler2D" and v.value is not None})

    class Moving(Basic):
        def build(self):
            Snapshot(scene=self)

        def update(self):
            self.camera.move(np.array([0.02, -0.01, 0.0]))
            self.camera.apply_zoom(0.05)
            self.camera.rotate2d(3.0)
            if self.frame_count == 3:
                self.camera.projection = CameraProjection.Stereoscopic
            self.frame_count += 1
        frame_count = 0

    w, h = 96, 54
    scene = Moving()
    raw = scene.main(width=w, height=h, fps=30, time=0.2, output=bytes)
    got = frames_of(raw, w, h)
    assert got.shape[0] == 6 and len(snapshots) == 6
    assert scene.camera.zoom.target == pytest.approx(1.05**6) and scene.camera.x == pytest.approx(scene.camera.position.value[0])
    for k, snap in enumerate(snapshots):
        u = O.default_uniforms(w, h)
        for name, value in snap.items():
            if hasattr(u, name):
                cur = getattr(u, name)
                if hasattr(cur, "__len__"):
                    for i in range(len(cur)):
                        cur[i] = float(value.ravel()[i])
                else:
                    setattr(u, name, type(cur)(value.ravel()[0]))
        want = O.resolve(O.render("default", u, {}, w, h, threads=4), w, h, 2)
        assert np.array_equal(got[k], want), (k, lsb_report(got[k], want))
    assert not np.array_equal(got[0], got[5])
    assert snapshots[5]["iCameraProjection"] == 1 and snapshots[2]["iCameraProjection"] == 0
    scene.camera.x = 0.5
    assert scene.camera.position.target[0] == 0.5
    assert np.allclose(scene.camera.left_target, -scene.camera.right_target) and np.allclose(scene.camera.backward_target, -scene.camera.forward_target)


def test_bench_prints_one_json_line_with_the_contract_fields():
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    out = subprocess.run([sys.executable, str(root/"bench.py"), "--steps", "2", "--warmup", "1", "--frames-per-step", "3",
                          "--width", "384", "--height", "216", "--cpu-seconds", "2", "--full"], capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [line for line in out.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1
    record = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "export_host"):
        assert key in record, key
    assert record["n_gpus"] == 1 and record["steps"] == 2 and record["warmup"] == 1 and record["unit"] == "frames/s"
    assert record["value"] > 0 and record["higher_is_better"] is True and record["scaling"] == "weak" and record["vs_baseline"] is None
    assert "workload" in record["config"] and "model" not in record["config"]
    # the binding roof of the dominant kernel is VALU issue; the HBM view of the contract sits beside it
    assert set(record["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "hbm"} and record["roofline"]["bound"] == "valu"
    assert set(record["roofline"]["hbm"]) >= {"achieved", "peak", "unit", "frac"} and record["roofline"]["hbm"]["unit"] == "GB/s"
    assert record["roofline"]["kernel"].startswith("k_")                      # at this size a run-time-sized tile of VisualizerShader; at 4K k_visualizer_fast
    assert set(record["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample", "single_thread"} and record["cpu_baseline"]["kind"] in ("port", "reference")
    assert record["cpu_baseline"]["single_thread"]["cores"] == 1 and record["export_host"]["value"] > 0


def test_plain_bench_run_measures_the_headline_only():
    """Without --full the line keeps its headline fields and measures nothing else: no CPU baseline, no export, no counter passes"""
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    out = subprocess.run([sys.executable, str(root/"bench.py"), "--steps", "2", "--warmup", "1", "--frames-per-step", "3",
                          "--width", "384", "--height", "216"], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [line for line in out.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1
    record = json.loads(lines[0])
    assert record["n_gpus"] == 1 and record["steps"] == 2 and record["warmup"] == 1 and record["unit"] == "frames/s" and record["dtype"] == "f32"
    assert record["value"] > 0 and record["ms_per_step"] > 0 and record["higher_is_better"] is True
    assert not {"cpu_baseline", "export_host", "value_host", "value_yuv420p"} & set(record), sorted(record)
    assert not (record["roofline"]["counters_from"] or "").startswith("live"), record["roofline"]["counters_from"]
    assert record["roofline"]["kernel"].startswith("k_") and record["roofline"]["launch_ms"] > 0


def test_bench_measures_the_instruction_counters_of_its_own_run():
    """The benchmark's configuration (C3) as the driver runs it, short: the dominant kernel's VALU counters come from two rocprofv3
    children of the run itself, and they say what the ISA census says (profiles/r05_strip_isa_census.txt) —
    549 instructions per supersample in rounds 3-4, 472 since round 5 packs the diagonal rows' red and green into v_pk_* forms (one
    instruction, two operations). Skipped where the profiler is not installed."""
    import json
    import shutil
    import subprocess
    import sys
    from pathlib import Path
    if shutil.which("rocprofv3") is None:
        pytest.skip("no rocprofv3 on this box")
    root = Path(__file__).resolve().parent.parent
    out = subprocess.run([sys.executable, str(root/"bench.py"), "--steps", "2", "--warmup", "1", "--frames-per-step", "30", "--full", "--no-cpu-baseline", "--no-export"],
                         capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    record = json.loads([line for line in out.stdout.splitlines() if line.startswith("{")][-1])
    roofline = record["roofline"]
    assert roofline["counters_from"].startswith("live: SQ_INSTS_VALU"), (roofline["counters_from"], out.stderr[-1500:])
    assert 385.0 < roofline["valu_instructions_per_supersample"] < 425.0, roofline      # (403 with round 6's pixel tier; 472 in round 5, 549 in rounds 3-4)
    assert 0.5 < roofline["issue_cycles_frac"] < 1.0 and 0.4 < roofline["frac"] < 0.8, roofline
    assert 1.8 < roofline["issue_model"]["effective_clock_GHz"] < 2.5, roofline["issue_model"]


@pytest.mark.parametrize("samplerate,fps,seconds", [(48000, 30.0, 0.4), (22050, 50.0, 0.3), (32000, 24.0, 0.5)])
def test_visualizer_other_sample_rates_and_frame_rates(samplerate, fps, seconds):
    """The chunk arithmetic, window schedule, filterbank and DynamicNumber coefficients all depend on (samplerate, fps): the tape and
    the frame loop against the oracle's audio + pixel pipeline for rates other than 44.1 kHz / 60 fps"""
    from examples.scenes import Visualizer, make
    w, h, ssaa = 112, 64, 2
    rng = np.random.default_rng(int(samplerate + fps))
    t = np.arange(int(samplerate*(seconds + 0.2)))/samplerate
    pcm = np.stack([0.6*np.sin(2*np.pi*(200 + 900*t)*t), 0.5*np.sin(2*np.pi*330*t) + 0.1*rng.standard_normal(len(t))], axis=1).astype(np.float32)
    background = synth.background_image(128, 72, seed=9)
    frames = round(seconds*fps)
    want = oracle_visualizer_frames(pcm, samplerate, background, w, h, ssaa, 2, fps, frames, seconds)
    for batch in (None, False):
        raw = make(Visualizer, audio=(pcm, samplerate), background=background).main(width=w, height=h, fps=fps, ssaa=ssaa, time=seconds, output=bytes, batch=batch)
        got = frames_of(raw, w, h)
        assert got.shape == want.shape
        mostly_within_one_lsb(got, want)


def test_host_api_odds_and_ends(tmp_path):
    """Pieces of the reference API surface that scenes use: scale/ratio in main (scene.py:493-561 + resolution.py), textures that
    track the scene at a factor, temporal writes/clears, swapping a fragment between exports, time given as an expression"""
    from examples.scenes import Basic
    from shaderflow_amd.shader import ShaderProgram
    from shaderflow_amd.texture import ShaderTexture

    scene = Basic()
    raw = scene.main(width=128, height=72, scale=0.5, fps=30, time="2/30", output=bytes)               # time strings are evaluated (scene.py:560)
    assert scene.resolution == (64, 36) and len(raw) == 2*64*36*3
    raw = Basic().main(height=90, ratio="16:9", fps=30, time=1/30, output=bytes)
    assert len(raw) == 160*90*3

    scene = Basic()
    scene.initialize()                                                                                  # modules need the scene's context (scene.py:128-195)
    half = ShaderProgram(scene=scene, name="half")
    half.texture.track = 0.5                                                                            # half the render resolution
    probe = ShaderTexture(scene=scene, name="probe", temporal=3, width=4, height=2, components=1, dtype=np.float32)
    scene.main(width=64, height=36, ssaa=2, fps=30, time=1/30, freewheel=True)
    assert half.texture.size == (64, 36) and scene.shader.texture.size == (128, 72) and scene._final.texture.size == (64, 36)
    data = np.arange(8, dtype=np.float32).reshape(2, 4, 1)
    probe.write(data, temporal=2)
    assert probe.is_empty(0) and not probe.is_empty(2) and np.array_equal(probe.matrix[2][0].texture.read(), data)
    probe.roll()
    assert np.array_equal(probe.matrix[0][0].texture.read(), data)                                      # deque.rotate(1): the last row comes first
    probe.clear(0)
    assert not probe.matrix[0][0].texture.read().any() and not probe.is_empty(0)
    probe.temporal = 2                                                                                  # shrinking re-allocates and keeps full writes of equal size
    assert len(probe.matrix) == 2

    scene = Basic()
    first = frames_of(scene.main(width=64, height=36, fps=30, time=1/30, output=bytes), 64, 36)
    assert scene.shader.kernel == "default"
    scene.shader.fragment = "shadertoy"                                                                 # hot swap (shader.py:299-306): compiled on the next export
    second = frames_of(scene.main(width=64, height=36, fps=30, time=1/30, output=bytes), 64, 36)
    assert scene.shader.kernel == "shadertoy" and not np.array_equal(first, second)
    scene.shader.fragment = "void main() { fragColor = vec4(0.2); }"                                     # not in the registry: translated and compiled
    third = frames_of(scene.main(width=64, height=36, fps=30, time=1/30, output=bytes), 64, 36)
    assert scene.shader.kernel == "translated" and not scene.shader.fallback and (third == 51).all()
    scene.shader.fragment = "void main() { fragColor = undeclared_function(stuv); }"                    # a compile error: missing.glsl (shader.py:323-340)
    scene.main(width=64, height=36, fps=30, time=1/30, freewheel=True)
    assert scene.shader.kernel == "missing" and scene.shader.fallback and "undeclared_function" in scene.shader.compile_error
    from shaderflow_amd.shader import ShaderDumper                                                      # the texts and the error are dumped (shader.py:68-73)
    dumped = ShaderDumper.directory()
    assert "undeclared_function" in (dumped/f"{scene.shader.uuid}.frag").read_text() and (dumped/f"{scene.shader.uuid}.hip").exists()
    assert "error" in (dumped/f"{scene.shader.uuid}-error.md").read_text()


def test_flac_and_wav_files_drive_the_same_export(tmp_path):
    """audio files reach ShaderAudio without an ffmpeg binary — RIFF/WAVE and FLAC through the native readers; the same
    samples in either container give the same frames, byte for byte"""
    import struct
    from examples.scenes import Visualizer, make
    from tests.flac_encoder import encode
    pcm, sr = clip(0.4)
    ints = np.clip(np.rint(pcm*32767.0), -32768, 32767).astype(np.int64)
    (tmp_path/"clip.flac").write_bytes(encode(ints, sr, 16, blocksize=4096, plan=lambda frame, channels: dict(assignment=10, subframes=[dict(kind="fixed", order=2, partition_order=3)]*2)))
    data = ints.astype("<i2").tobytes()
    (tmp_path/"clip.wav").write_bytes(struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, 1, 2, sr, sr*4, 4, 16, b"data", len(data)) + data)
    background = synth.background_image(96, 54, seed=3)
    kw = dict(width=96, height=54, fps=60.0, ssaa=2, time=0.25, output=bytes)
    from_flac = make(Visualizer, audio=str(tmp_path/"clip.flac"), background=background).main(**kw)
    from_wav = make(Visualizer, audio=str(tmp_path/"clip.wav"), background=background).main(**kw)
    assert from_flac == from_wav and frames_of(from_flac, 96, 54).std() > 1


def test_set_uniform_between_frames_is_not_masked_by_the_pipeline_cache():
    """ShaderProgram answers an unchanged pipeline value from its last python value; a value set through set_uniform() in between
    has to invalidate that answer, or the next (unchanged) pipeline push would leave set_uniform's value on the device"""
    from examples.scenes import Basic
    scene = Basic()
    scene.initialize()
    scene.relay(__import__("shaderflow_amd.message", fromlist=["ShaderMessage"]).ShaderMessage.Shader.Compile)
    program = scene.shader
    program.compile()
    assert program._push("iTime", 1.5, "float") is not None
    assert program._pushed_plain["iTime"][1] == 1.5
    program.set_uniform("iTime", 9.0)                                 # another route to the same uniform
    assert "iTime" not in program._pushed_plain
    sent_before = program._pushed["iTime"]
    program._push("iTime", 1.5, "float")                              # the pipeline's unchanged value must reach the device again
    assert program._pushed["iTime"] != sent_before and program._pushed_plain["iTime"][1] == 1.5


def test_mipmaps_follow_the_references_build_order():
    """SURVEY §8 P1 (texture.py:116-137, 274-283; whole-image parity: tests/test_gpu_mip.py). Observable rules of the reference kept:
    `mipmaps=True` makes apply() rebuild the chain from the CURRENT level 0; write() touches level 0 only; from_numpy() runs
    make() → apply() before its write, so the chain of a texture that is only ever filled that way is the chain of zeros."""
    from examples.scenes import Basic
    from shaderflow_amd.texture import ShaderTexture
    scene = Basic()
    scene.initialize()
    data = np.full((8, 8, 4), 200, np.uint8)
    texture = ShaderTexture(scene=scene, name="mipmapped", mipmaps=True, anisotropy=16).from_numpy(data)
    box = texture.get_box().texture
    assert np.array_equal(box.read_level(0), data) and not box.read_level(1).any()      # level 0 written after the chain was built
    texture.repeat(False)                                                               # apply(): the chain of the data
    assert (box.read_level(1) == 200).all() and (box.read_level(3) == 200).all() and box.read_level(3).shape == (1, 1, 4)
    texture.write(np.zeros((8, 8, 4), np.uint8))
    assert not box.read_level(0).any() and (box.read_level(1) == 200).all()             # … and stale again after the next write
    plain = ShaderTexture(scene=scene, name="plain").from_numpy(data)
    plain.mipmaps = True                                                                # the setter applies (texture.py:116): the chain of the data
    assert (plain.get_box().texture.read_level(2) == 200).all()
