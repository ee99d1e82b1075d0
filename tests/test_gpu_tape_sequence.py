"""
TapeSequence (shaderflow_amd/tapesequence.py): audio-reactive layered, temporal and multi-program scenes without python logic are drawn
by the native sequence from the device audio tape, and every frame equals the frame loop's (`main(batch=False)`) byte for byte.
"""
from __future__ import annotations

import numpy as np
import pytest

from shaderflow_amd import synth

pytestmark = pytest.mark.gpu

FPS = 60.0
W, H = 160, 90
PCM = None


def clip():
    global PCM
    if PCM is None:
        PCM = synth.sweep_clip(4.0, 44100)
    return PCM


def render(scene, frames, batch, ssaa=1.0, pixel_format=None):
    raw = scene.main(width=W, height=H, fps=FPS, ssaa=ssaa, subsample=2, time=frames/FPS, output=bytes, batch=batch, pixel_format=pixel_format)
    per_frame = W*H*3//2 if pixel_format == "yuv420p" else W*H*3
    assert len(raw) == frames*per_frame
    return np.frombuffer(raw, np.uint8).reshape(frames, per_frame)


def assert_frames_equal(loop, tape):
    assert loop.shape == tape.shape
    for k in range(loop.shape[0]):
        assert np.array_equal(loop[k], tape[k]), f"frame {k} differs"


# ---- the scenes -------------------------------------------------------------------------------------------------------------------

def trails():
    from examples.scenes import AudioTrails

    class Trails(AudioTrails):
        audio_source = (clip(), 44100)
    return Trails


def two_programs():
    """A child program that draws the spectrum (samples iSpectrogram), composited by the main one, which reads the volume: the main
    pass is fused into iFinal, from the tape"""
    from examples.scenes import _AudioScene
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    from shaderflow_amd.shader import ShaderProgram

    class TwoPrograms(_AudioScene):
        audio_source = (clip(), 44100)

        def build(self):
            self._load_audio()
            self.spectrogram = ShaderSpectrogram(scene=self, length=0, audio=self.audio)
            self.spectrogram.from_notes(start="C2", end="C7", bins=64)
            self.child = ShaderProgram(scene=self, name="child")
            self.child.fragment = ("void main() { vec2 s = texture(iSpectrogram, vec2(0.5, astuv.x)).xy;\n"
                                   "    fragColor = vec4(step(astuv.y, sqrt(s.x)/60.0), step(astuv.y, sqrt(s.y)/60.0), astuv.x, 1.0); }")
            self.shader.fragment = ("void main() { vec3 c = texture(child, astuv).rgb;\n"
                                    "    fragColor = vec4(c*(0.5 + iAudioVolume) + vec3(0.1*iAudioSTD, 0.0, 0.2*fract(iTime)), 1.0); }")
    return TwoPrograms


def temporal_visualizer():
    from examples.scenes import Visualizer

    class Temporal(Visualizer):
        audio_source = (clip(), 44100)
        background = synth.background_image(240, 135, seed=5)

        def build(self):
            Visualizer.build(self)
            self.shader.texture.temporal = 4
    return Temporal


def scrolling_layers():
    from examples.scenes import _AudioScene
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram

    class Scrolling(_AudioScene):
        audio_source = (clip(), 44100)

        def build(self):
            self._load_audio()
            self.spectrogram = ShaderSpectrogram(scene=self, length=0.5, audio=self.audio)
            self.spectrogram.from_notes(start="C2", end="C7", bins=64)
            self.shader.texture.layers = 2
            self.shader.fragment = (
                "void main() {\n"
                "    if (iLayer == 0) { vec2 s = texture(iSpectrogram, vec2(fract(astuv.x + iSpectrogramOffset), astuv.y)).xy;\n"
                "        fragColor = vec4(sqrt(s)/40.0, 0.5*iAudioVolume, 1.0); return; }\n"
                "    vec4 now = texture(iScreen0x0, astuv);\n"
                "    fragColor = vec4(now.rg, now.b + 0.25*astuv.y, 1.0);\n"
                "}\n")
    return Scrolling


def waveform_trail():
    from examples.scenes import _AudioScene
    from shaderflow_amd.audio.waveform import ShaderWaveform

    class WaveTrail(_AudioScene):
        audio_source = (clip(), 44100)

        def build(self):
            self._load_audio()
            self.waveform = ShaderWaveform(scene=self, audio=self.audio)
            self.shader.texture.temporal = 2
            self.shader.fragment = (
                "void main() {\n"
                "    vec2 w = texture(iWaveform, vec2(astuv.x, 0.0)).xy;\n"
                "    float line = step(abs(gluv.y - w.x), 0.05) + step(abs(gluv.y - w.y), 0.05);\n"
                "    vec3 before = iScreenTexture(1, 0, astuv).rgb;\n"
                "    fragColor = vec4(max(vec3(line, 0.5*line, 0.25), 0.9*before), 1.0);\n"
                "}\n")
    return WaveTrail


SCENES = {"trails": trails, "two-programs": two_programs, "temporal-visualizer": temporal_visualizer,
          "scrolling-layers": scrolling_layers, "waveform": waveform_trail}


# ---- byte equality with the frame loop --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ssaa", [1.0, 2.0])
@pytest.mark.parametrize("case", list(SCENES))
def test_tape_sequence_gives_the_frame_loops_bytes(case, ssaa):
    Scene = SCENES[case]()
    frames = 150                                                   # three batches of 60
    want = render(Scene(), frames, batch=False, ssaa=ssaa)
    scene = Scene()
    got = render(scene, frames, batch=None, ssaa=ssaa)
    assert scene.tape_sequence is not None and scene.tape_sequence.frames == frames
    assert scene.tape_loop is None
    assert_frames_equal(want, got)


def test_chunks_of_three_frames_inside_the_temporal_history(monkeypatch):
    from shaderflow_amd.clockloop import ClockLoop
    Scene = trails()
    frames = 150
    want = render(Scene(), frames, batch=False, ssaa=2.0)
    sizes = []

    def three(self, measured):
        sizes.append(3)
        return 3
    monkeypatch.setattr(ClockLoop, "chunk_frames", three)
    scene = Scene()
    got = render(scene, frames, batch=None, ssaa=2.0)
    assert scene.tape_sequence is not None and len(sizes) >= frames//3
    assert_frames_equal(want, got)


def test_yuv420p_matches_the_frame_loop():
    Scene = trails()
    frames = 150
    want = render(Scene(), frames, batch=False, pixel_format="yuv420p")
    scene = Scene()
    got = render(scene, frames, batch=None, pixel_format="yuv420p")
    assert scene.tape_sequence is not None
    assert_frames_equal(want, got)


# ---- the path is really taken ------------------------------------------------------------------------------------------------------

def test_trails_run_on_the_tape_without_host_audio(monkeypatch):
    from shaderflow_amd.audio.module import ShaderAudio
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    Scene = trails()
    frames = 150
    want = render(Scene(), frames, batch=False, ssaa=1.0)

    def forbidden(*args, **kwargs):
        raise AssertionError("per-frame host audio ran under TapeSequence")
    monkeypatch.setattr(ShaderSpectrogram, "next", forbidden)
    monkeypatch.setattr(ShaderAudio, "loudness_targets", forbidden)
    scene = Scene()
    got = render(scene, frames, batch=None, ssaa=1.0)
    assert scene.tape_sequence is not None
    assert_frames_equal(want, got)


# ---- ineligible scenes keep their loop ---------------------------------------------------------------------------------------------

def test_ineligible_scenes_take_the_frame_loop(monkeypatch):
    Trails = trails()

    class Scripted(Trails):
        counted = 0

        def update(self):
            self.counted += 1

    class Rolled(Trails):
        def build(self):
            Trails.build(self)
            target = np.array(self.camera.position.target, dtype=np.float64)
            target[-1] += 0.3
            self.camera.position.set(target)                       # at rest, away from the identity pose

    frames = 6
    for cls in (Scripted, Rolled):
        scene = cls()
        want = render(cls(), frames, batch=False)
        got = render(scene, frames, batch=None)
        assert scene.tape_sequence is None and scene.tape_loop is None, cls.__name__
        assert_frames_equal(want, got)
    monkeypatch.setenv("SHADERFLOW_TAPE_SEQUENCE", "0")
    scene = Trails()
    render(scene, frames, batch=None)
    assert scene.tape_sequence is None and scene.tape_loop is None
    monkeypatch.delenv("SHADERFLOW_TAPE_SEQUENCE")
    scene = Trails()
    render(scene, frames, batch=None)
    assert scene.tape_sequence is not None


def test_scenes_of_the_other_loops_keep_them(monkeypatch):
    from examples.scenes import MotionBlur, Visualizer, make
    from shaderflow_amd.clockloop import ClockLoop
    from shaderflow_amd.tape import FrameTape
    taken = []
    for cls, name in ((FrameTape, "export"), (ClockLoop, "run")):
        original = getattr(cls, name)

        def spy(self, *args, _original=original, _cls=cls, **kwargs):
            taken.append(_cls.__name__)
            return _original(self, *args, **kwargs)
        monkeypatch.setattr(cls, name, spy)
    frames = 6
    scene = make(Visualizer, audio=(clip(), 44100), background=synth.background_image(240, 135, seed=6))
    render(scene, frames, batch=None)
    assert taken == ["FrameTape"] and scene.tape_sequence is None
    scene = make(MotionBlur, background=synth.background_image(240, 135, seed=7))
    render(scene, frames, batch=None)
    assert taken == ["FrameTape", "ClockLoop"] and scene.tape_sequence is None

    class Counting(Visualizer):
        audio_source = (clip(), 44100)
        background = synth.background_image(240, 135, seed=3)
        counted = 0

        def update(self):
            self.counted += 1
    scene = Counting()
    render(scene, frames, batch=None)
    assert scene.tape_loop is not None and scene.tape_sequence is None and scene.counted == frames


# ---- host state after an export ----------------------------------------------------------------------------------------------------

def test_host_state_after_the_run_is_the_frame_tapes():
    from examples.scenes import Visualizer
    frames = 75

    class Stock(Visualizer):
        audio_source = (clip(), 44100)
        background = synth.background_image(240, 135, seed=8)
    reference, scene = Stock(), trails()()
    render(reference, frames, batch=None)                          # FrameTape.export
    render(scene, frames, batch=None)
    assert scene.tape_sequence is not None and reference.tape_sequence is None
    assert (scene.time, scene.dt, scene.rdt) == (reference.time, reference.dt, reference.rdt)
    assert scene.audio.tell == reference.audio.tell
    for mine, theirs in ((scene.audio.volume, reference.audio.volume), (scene.audio.std, reference.audio.std),
                         (scene.spectrogram.dynamics, reference.spectrogram.dynamics)):
        for field in ("value", "target", "integral", "derivative"):
            assert np.array_equal(np.asarray(getattr(mine, field)), np.asarray(getattr(theirs, field))), field
