"""
TapeLoop (shaderflow_amd/tapeloop.py): audio scenes with update() logic of their own take the device audio tape, and every frame
equals the frame loop's (`main(batch=False)`) byte for byte.
"""
from __future__ import annotations

import numpy as np
import pytest

from shaderflow_amd import synth

pytestmark = pytest.mark.gpu

FPS = 60.0
PCM = None


def clip():
    global PCM
    if PCM is None:
        PCM = synth.sweep_clip(4.0, 44100)
    return PCM


def render(scene, frames, w, h, batch, ssaa=1.0):
    raw = scene.main(width=w, height=h, fps=FPS, ssaa=ssaa, subsample=2, time=frames/FPS, output=bytes, batch=batch)
    return np.frombuffer(raw, np.uint8).reshape(frames, h, w, 3)


def counting_visualizer():
    from examples.scenes import Visualizer

    class Counting(Visualizer):
        audio_source = (clip(), 44100)
        background = synth.background_image(240, 135, seed=3)
        counted = 0

        def update(self):
            self.counted += 1
    return Counting


def assert_frames_equal(loop, tape):
    assert loop.shape == tape.shape
    for k in range(loop.shape[0]):
        assert np.array_equal(loop[k], tape[k]), f"frame {k} differs"


@pytest.mark.parametrize("ssaa", [1.0, 2.0])
def test_counting_visualizer_runs_on_the_tape_without_host_audio(ssaa, monkeypatch):
    from shaderflow_amd.audio.module import ShaderAudio
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    Counting = counting_visualizer()
    frames = 150                                                   # three batches of 60
    want = render(Counting(), frames, 320, 180, batch=False, ssaa=ssaa)

    def forbidden(*args, **kwargs):
        raise AssertionError("per-frame host audio ran under TapeLoop")
    monkeypatch.setattr(ShaderSpectrogram, "next", forbidden)
    monkeypatch.setattr(ShaderAudio, "loudness_targets", forbidden)
    scene = Counting()
    got = render(scene, frames, 320, 180, batch=None, ssaa=ssaa)
    assert scene.tape_loop is not None and scene.tape_loop.frames_mirrored == frames
    assert scene.counted == frames
    assert_frames_equal(want, got)


PROBE = """
void main() {
    vec2 v = (stuv.x < 0.5) ? iBefore : iAfter;
    float x = (stuv.y < 0.5) ? v.x : v.y;
    fragColor = vec4(fract(x*97.0), fract(x*13.0), x*4.0, 1.0);
}
"""


def probe_scene(length=0.0):
    from shaderflow_amd.audio import ShaderAudio
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    from shaderflow_amd.module import ShaderModule
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.variable import Uniform

    class Reader(ShaderModule):
        uniform = "iBefore"
        seen: list = None

        def update(self):
            scene = self.scene
            value = (float(scene.audio.volume.value), float(np.asarray(scene.spectrogram.dynamics.value).reshape(-1)[3])
                     if np.asarray(scene.spectrogram.dynamics.value).size > 3 else 0.0)
            self.seen = (self.seen or []) + [value]
            self.current = value

        def pipeline(self):
            yield Uniform("vec2", self.uniform, getattr(self, "current", (0.0, 0.0)))

    class Probe(ShaderScene):
        def build(self):
            self.before = Reader(scene=self)
            self.audio = ShaderAudio(scene=self, name="iAudio")
            self.audio.load(samples=clip(), samplerate=44100)
            self.spectrogram = ShaderSpectrogram(scene=self, length=length, audio=self.audio)
            self.spectrogram.from_notes(start="C2", end="C7", bins=64)
            self.after = Reader(scene=self)
            self.after.uniform = "iAfter"
            self.shader.fragment = PROBE
    return Probe


def test_user_modules_see_the_mirrored_audio_state_in_order():
    Probe = probe_scene()
    frames = 130
    loop_scene, tape_scene = Probe(), Probe()
    want = render(loop_scene, frames, 160, 90, batch=False)
    got = render(tape_scene, frames, 160, 90, batch=None)
    assert tape_scene.tape_loop is not None and tape_scene.tape_loop.frames_mirrored == frames
    assert tape_scene.before.seen == loop_scene.before.seen        # frame k-1's values, bit for bit
    assert tape_scene.after.seen == loop_scene.after.seen          # frame k's
    assert tape_scene.before.seen[5] != tape_scene.after.seen[5]
    # every field of every mirrored system, dtypes included, as the frame loop leaves it
    from shaderflow_amd.tapeloop import _dynamics_state
    for name in ("volume", "std"):
        assert _dynamics_state(getattr(tape_scene.audio, name)) == _dynamics_state(getattr(loop_scene.audio, name)), name
    assert _dynamics_state(tape_scene.spectrogram.dynamics) == _dynamics_state(loop_scene.spectrogram.dynamics)
    assert (tape_scene.audio.tell, tape_scene.spectrogram.offset) == (loop_scene.audio.tell, loop_scene.spectrogram.offset)
    assert np.array_equal(tape_scene.audio.data, loop_scene.audio.data)
    assert_frames_equal(want, got)


def driven_visualizer(camera: str):
    from examples.scenes import Visualizer
    from shaderflow_amd.dynamics import ShaderDynamics

    class Driven(Visualizer):
        audio_source = (clip(), 44100)
        background = synth.background_image(240, 135, seed=4)

        def build(self):
            Visualizer.build(self)
            self.push = ShaderDynamics(scene=self, name="iPush", frequency=3, zeta=0.6, value=0.0)

        def update(self):
            self.push.target = float(self.audio.volume.value)*3.0          # a demo.py-style ShaderDynamics driven from update()
            if camera == "static" and self.frame == 0:
                target = np.array(self.camera.position.target, dtype=np.float64)
                target[-1] += 0.3
                self.camera.position.set(target)
            if camera == "moving" and 20 <= self.frame < 50:
                target = np.array(self.camera.position.target, dtype=np.float64)
                target[-1] += 0.01*float(self.push.value)
                self.camera.position.target = target
    return Driven


def test_dynamics_driven_from_update_stay_on_the_tape():
    Driven = driven_visualizer("none")
    frames = 90
    want = render(Driven(), frames, 320, 180, batch=False, ssaa=2.0)
    scene = Driven()
    got = render(scene, frames, 320, 180, batch=None, ssaa=2.0)
    assert scene.tape_loop is not None and scene.tape_loop.frames_mirrored == frames
    assert_frames_equal(want, got)


@pytest.mark.parametrize("camera", ["moving", "static"])
def test_a_camera_away_from_identity_takes_the_frame_loop(camera):
    # (a non-identity camera lets the tape launch and the frame loop's launch pick different visualizer configurations: tapeloop.py
    # camera_at_identity) — a camera moved from frame 20 hands the rest over there, one posed before the first frame the whole export
    Driven = driven_visualizer(camera)
    frames = 70
    want = render(Driven(), frames, 320, 180, batch=False, ssaa=2.0)
    scene = Driven()
    got = render(scene, frames, 320, 180, batch=None, ssaa=2.0)
    assert scene.tape_loop is not None
    if camera == "moving":
        assert 20 <= scene.tape_loop.frames_mirrored < frames
    else:
        assert scene.tape_loop.frames_mirrored == 0
    assert_frames_equal(want, got)


@pytest.mark.parametrize("case", ["frequency@37", "volume@50", "frequency@37-scrolling"])
def test_writes_to_the_audio_state_switch_to_the_frame_loop(case):
    what, _, at = case.partition("@")
    at, scrolling = int(at.split("-")[0]), at.endswith("scrolling")
    Base = probe_scene(length=0.5 if scrolling else 0.0)
    scroll = "" if not scrolling else "fragColor.rg += texture(iSpectrogram, astuv).rg*20.0;"
    fragment = PROBE.replace("fragColor = vec4(fract(x*97.0), fract(x*13.0), x*4.0, 1.0);",
                             "fragColor = vec4(fract(x*97.0), fract(x*13.0), x*4.0, 1.0);" + scroll)

    class Writer(Base):
        def build(self):
            Base.build(self)
            self.shader.fragment = fragment

        def update(self):
            if self.frame == at:
                if what == "frequency":
                    self.spectrogram.dynamics.frequency = 9.0
                else:
                    self.audio.volume.value = np.array(0.75)
    frames = 90
    want = render(Writer(), frames, 160, 90, batch=False)
    scene = Writer()
    got = render(scene, frames, 160, 90, batch=None)
    assert scene.tape_loop is not None and scene.tape_loop.frames_mirrored == at
    assert_frames_equal(want, got)


def test_background_rewrites_and_screenshot_mid_batch():
    from examples.scenes import Visualizer
    images = [synth.background_image(240, 135, seed=s) for s in range(6)]

    class Slides(Visualizer):
        audio_source = (clip(), 44100)
        background = images[0]
        shot = None

        def update(self):
            if self.frame % 20 == 0:
                self.back.from_numpy(images[(self.frame//20) % len(images)])
            if self.frame == 30:
                self.shot = self.screenshot()
    frames = 100
    loop_scene, tape_scene = Slides(), Slides()
    want = render(loop_scene, frames, 320, 180, batch=False, ssaa=2.0)
    got = render(tape_scene, frames, 320, 180, batch=None, ssaa=2.0)
    assert tape_scene.tape_loop is not None and tape_scene.tape_loop.frames_mirrored == frames
    assert_frames_equal(want, got)
    assert np.array_equal(loop_scene.shot, tape_scene.shot)
    assert np.array_equal(tape_scene.shot, got[29][::-1])          # (the raw stream holds rows bottom-up)
    assert np.array_equal(loop_scene.screenshot(), tape_scene.screenshot())


def test_snapshot_read_requires_opt_in_before_the_first_build():
    import ctypes as C

    from examples.scenes import Visualizer, make
    from shaderflow_amd import _native as N
    from shaderflow_amd.tape import FrameTape
    scene = make(Visualizer, audio=(clip(), 44100), background=synth.background_image(64, 36))
    scene.main(width=64, height=36, fps=FPS, time=2/FPS, freewheel=True, batch=False)
    tape = FrameTape(scene).prepare(8)
    raw = np.zeros(1 << 20, np.uint8)
    assert N.lib().sfx_tape_read(tape.handle, N.TAPE_STATE, 0, 1, raw.ctypes.data, C.c_size_t(96 + 24*tape.spectrogram.spectrogram_bins*2)) != 0
    tape.build(0, 8)
    assert N.lib().sfx_tape_snapshot(tape.handle, 1) != 0          # too late: the acceleration state was not kept
    tape.release()


def test_ineligible_scenes_take_the_frame_loop(monkeypatch):
    from shaderflow_amd.audio import ShaderAudio
    from shaderflow_amd.shader import ShaderProgram
    Counting = counting_visualizer()

    class ExtraProgram(Counting):
        def build(self):
            Counting.build(self)
            self.child = ShaderProgram(scene=self, name="child")
            self.child.fragment = "void main() { fragColor = vec4(astuv.x, 0.25, 0.5, 1.0); }"

    class MyAudio(ShaderAudio):
        pass

    class SubclassedAudio(Counting):
        def _load_audio(self):
            self.audio = MyAudio(scene=self, name="iAudio")
            self.audio.load(samples=clip(), samplerate=44100)

    for cls in (ExtraProgram, SubclassedAudio):
        scene = cls()
        render(scene, 6, 64, 36, batch=None)
        assert scene.tape_loop is None, cls.__name__
    monkeypatch.setenv("SHADERFLOW_TAPE_LOOP", "0")
    scene = Counting()
    render(scene, 6, 64, 36, batch=None)
    assert scene.tape_loop is None
    monkeypatch.delenv("SHADERFLOW_TAPE_LOOP")
    scene = Counting()
    render(scene, 6, 64, 36, batch=None)
    assert scene.tape_loop is not None and scene.tape_loop.frames_mirrored == 6


def test_4k_counting_visualizer_matches_the_frame_loop():
    Counting = counting_visualizer()
    frames = 12
    want = render(Counting(), frames, 3840, 2160, batch=False, ssaa=1.0)
    scene = Counting()
    got = render(scene, frames, 3840, 2160, batch=None, ssaa=1.0)
    assert scene.tape_loop is not None
    assert_frames_equal(want, got)
