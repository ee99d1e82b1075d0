"""
The piano-and-tape sequence (shaderflow_amd/sequence.py): a piano roll beside audio modules, without python logic, is drawn by ONE native
sequence that names the piano and the audio tape, and every frame equals the frame loop's (`ShaderScene.next`) byte for byte.

The frame loop here is the real one: `SHADERFLOW_PIANO_TAPE=0` alone would hand a single-program scene of this kind to the tape loop
(tapeloop.py takes it: the piano is python logic to it), so the reference runs switch `SHADERFLOW_TAPE_LOOP` off as well and check that
no loop object was left on the scene.

  1. the PianoAudio example against the frame loop: frames, clock, the piano's host state and textures;
  2. the layered route (a temporal main texture that reads the piano, the spectrum and its own history) and a two-program scene whose
     child reads the piano only;
  3. chunks that never end where the tape's batches end;
  4. a piano under another name;
  5. no `update()` of the piano or the audio modules runs;
  6. a run that fails leaves the host objects at the last frame drawn;
  7. scenes the sequence does not take keep their loop and their frames;
  8. the other loops keep their scenes;
  9. the descriptor's validation is still in force with a piano beside a tape.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from shaderflow_amd import synth
from shaderflow_amd.piano import PianoNote

pytestmark = pytest.mark.gpu

FPS = 60.0
W, H = 160, 90
SECONDS = 4.0
STATE = ("value", "target", "previous", "derivative", "acceleration")
SWITCHES = ("SHADERFLOW_PIANO_TAPE", "SHADERFLOW_PIANO_SEQUENCE", "SHADERFLOW_TAPE_SEQUENCE")
PCM = None


def score():
    from examples.scenes import demo_score
    return demo_score(SECONDS)


def clip():
    """Four seconds of the score's own sound, made once"""
    global PCM
    if PCM is None:
        PCM = synth.score_clip(score(), SECONDS)
    return PCM


def render(scene, frames, ssaa=1.0, pixel_format=None):
    raw = scene.main(width=W, height=H, fps=FPS, ssaa=ssaa, subsample=2, time=frames/FPS, output=bytes, pixel_format=pixel_format)
    per_frame = W*H*3//2 if pixel_format == "yuv420p" else W*H*3
    assert len(raw) == frames*per_frame
    return np.frombuffer(raw, np.uint8).reshape(frames, per_frame)


def frame_loop(Scene, frames, monkeypatch, **kwargs):
    """(scene, frames) of `Scene` drawn by ShaderScene.next"""
    monkeypatch.setenv("SHADERFLOW_PIANO_TAPE", "0")
    monkeypatch.setenv("SHADERFLOW_TAPE_LOOP", "0")
    scene = Scene()
    out = render(scene, frames, **kwargs)
    assert scene.piano_tape is None and scene.piano_sequence is None and scene.tape_sequence is None and scene.tape_loop is None
    monkeypatch.delenv("SHADERFLOW_PIANO_TAPE")
    monkeypatch.delenv("SHADERFLOW_TAPE_LOOP")
    return scene, out


def assert_frames_equal(loop, sequence):
    assert loop.shape == sequence.shape
    for k in range(loop.shape[0]):
        assert np.array_equal(loop[k], sequence[k]), f"frame {k} differs"


def textures(piano):
    """(keys (128,), channels (128,), roll (128, 256, 4)) as the device holds them"""
    return (piano.keys_texture.texture.read()[0, :, 0].copy(), piano.channel_texture.texture.read()[0, :, 0].copy(),
            piano.roll_texture.texture.read().copy())


def assert_same_piano(loop, scene):
    """Both DynamicNumbers field by field, the three textures and the roll's host copy"""
    for name in STATE:
        assert np.array_equal(getattr(loop.piano.key_press_dynamics, name), getattr(scene.piano.key_press_dynamics, name)), f"key_press_dynamics.{name}"
        assert np.array_equal(getattr(loop.piano.note_range_dynamics, name), getattr(scene.piano.note_range_dynamics, name)), f"note_range_dynamics.{name}"
    for what, a, b in zip(("iPianoKeys", "iPianoChan", "iPianoRoll"), textures(loop.piano), textures(scene.piano)):
        assert np.array_equal(a, b), what
    assert scene.piano.roll_texture.get_box().data == loop.piano.roll_texture.get_box().data


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------

def piano_audio():
    from examples.scenes import PianoAudio

    class Scene(PianoAudio):
        score = score()
        audio_source = (clip(), 44100)
    return Scene


class _Parts:
    """What the scenes below share: a piano with the score, the clip, a spectrogram of it"""

    def add_piano(self, name="iPiano", notes=None, kind=None):
        from shaderflow_amd.piano import ShaderPiano
        piano = (kind or ShaderPiano)(scene=self, name=name)
        for note in (score() if notes is None else notes):
            piano.add_note(note)
        return piano

    def add_audio(self, kind=None):
        from shaderflow_amd.audio import ShaderAudio
        from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
        self.audio = ShaderAudio(scene=self, name="iAudio")
        self.audio.load(samples=clip(), samplerate=44100)
        self.spectrogram = (kind or ShaderSpectrogram)(scene=self, length=0, audio=self.audio)
        self.spectrogram.from_notes(start="C2", end="C7", bins=64)


TRAILS = """
    void main() {
        int note = int(floor(astuv.x*128.0));
        vec4 entry = texelFetch(iPianoRoll, ivec2(0, note), 0);
        float sounds = (entry.w > 0.0 && iTime >= entry.x && iTime <= entry.y) ? 1.0 : 0.35;
        vec2 s = texture(iSpectrogram, vec2(0.5, astuv.x)).xy;
        float level = clamp(sqrt(max(0.5*(s.x + s.y), 0.0))/30.0, 0.0, 1.0);
        vec3 now = vec3(step(astuv.y, level), sounds*entry.w/127.0*step(0.5, astuv.y), 0.2*fract(iTime));
        vec3 before = 0.6*iScreenTexture(1, 0, astuv).rgb + 0.3*iScreenTexture(3, 0, astuv).rgb;
        fragColor = vec4(max(now, before), 1.0);
    }
"""

CHILD = """
    void main() {
        int note = int(floor(astuv.x*128.0));
        float pressed = clamp(texelFetch(iPianoKeys, ivec2(note, 0), 0).x/100.0, 0.0, 1.0);
        vec4 entry = texelFetch(iPianoRoll, ivec2(0, note), 0);
        fragColor = vec4(pressed, entry.w/127.0, step(astuv.y, entry.y - entry.x), 1.0);
    }
"""

MAIN = """
    void main() {
        vec3 c = texture(child, astuv).rgb;
        float inside = step(iPianoDynamic.x/128.0, astuv.x)*step(astuv.x, (iPianoDynamic.y + 1.0)/128.0);
        fragColor = vec4(c*(0.4 + iAudioVolume) + vec3(0.0, 0.0, 0.3*inside*(0.5 + 0.5*fract(iTime))), 1.0);
    }
"""


def temporal_trails():
    """The audio pass is a layered one: its texture has history, so it is drawn into row 0 through render_box, from the tape"""
    from shaderflow_amd.scene import ShaderScene

    class Trails(_Parts, ShaderScene):
        def build(self):
            self.piano = self.add_piano()
            self.add_audio()
            self.shader.texture.temporal = 4
            self.shader.fragment = TRAILS
    return Trails


def two_programs():
    """The child reads the piano and no audio: drawn without the tape. The main program composites it and reads the volume and the note
    range: fused into iFinal, from the tape, where the fused kernel applies"""
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.shader import ShaderProgram

    class TwoPrograms(_Parts, ShaderScene):
        def build(self):
            # a note far behind the run widens the global range, so the note range travels towards the notes at hand
            self.piano = self.add_piano(notes=[*score(), PianoNote(note=100, start=30.0, end=30.5, channel=2, velocity=90)])
            self.add_audio()
            self.child = ShaderProgram(scene=self, name="child")
            self.child.fragment = CHILD
            self.shader.fragment = MAIN
    return TwoPrograms


# ---- 1. the example against the frame loop -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pixel_format", ["rgb24", "yuv420p"])
@pytest.mark.parametrize("ssaa", [1.0, 2.0])
def test_piano_tape_gives_the_frame_loops_bytes(ssaa, pixel_format, monkeypatch):
    Scene, frames = piano_audio(), 75                                   # across the tape's batch of 60, in several chunks
    loop, want = frame_loop(Scene, frames, monkeypatch, ssaa=ssaa, pixel_format=pixel_format)
    scene = Scene()
    got = render(scene, frames, ssaa=ssaa, pixel_format=pixel_format)
    assert scene.piano_tape is not None and scene.piano_tape.frames == frames
    assert scene.piano_sequence is None and scene.tape_sequence is None and scene.tape_loop is None
    assert scene.shader.translated and not scene.shader.fallback
    assert_frames_equal(want, got)
    assert len({frame.tobytes() for frame in got}) > frames//2         # the picture moves
    assert (scene.time, scene.dt, scene.rdt) == (loop.time, loop.dt, loop.rdt)
    assert_same_piano(loop, scene)
    assert scene.piano.key_press_dynamics.value.any() and textures(scene.piano)[2].any()


def test_the_picture_shows_the_sound(monkeypatch):
    """The strip under the keyboard and the glow come from the audio: the same score over silence is another picture there"""
    from examples.scenes import PianoAudio, make
    frames = 40
    scene = piano_audio()()
    played = render(scene, frames)
    silent_scene = make(PianoAudio, score=score(), audio=(np.zeros_like(clip()), 44100))
    silent = render(silent_scene, frames)
    assert scene.piano_tape is not None and silent_scene.piano_tape is not None
    picture, quiet = played[-1].reshape(H, W, 3), silent[-1].reshape(H, W, 3)      # rows bottom-up
    roll = int(scene.piano.height*H) + 1
    assert not np.array_equal(picture[:roll - 2], quiet[:roll - 2])                 # the spectrum strip and the glowing keys
    differing = np.flatnonzero((picture != quiet).any(axis=(1, 2)))
    assert differing.max() < roll + 2, differing                                    # the falling notes do not listen (the resolve's taps reach a row or two up)


# ---- 2. the layered route, and a pass that reads the piano only ------------------------------------------------------------------------

@pytest.mark.parametrize("ssaa", [1.0, 2.0])
@pytest.mark.parametrize("case", ["temporal", "two-programs"])
def test_layered_and_multi_program_scenes(case, ssaa, monkeypatch):
    Scene, frames = {"temporal": temporal_trails, "two-programs": two_programs}[case](), 75
    loop, want = frame_loop(Scene, frames, monkeypatch, ssaa=ssaa)
    scene = Scene()
    got = render(scene, frames, ssaa=ssaa)
    assert scene.piano_tape is not None and scene.piano_tape.frames == frames
    assert all(program.translated and not program.fallback for program in scene.piano_tape.clock.programs if not program.texture.final)
    assert_frames_equal(want, got)
    assert len({frame.tobytes() for frame in got}) > frames//2
    assert_same_piano(loop, scene)
    if case == "two-programs":                                          # the note range did travel: each frame was drawn with its own
        first = np.array([scene.piano.global_minimum_note, scene.piano.global_maximum_note], np.float32)
        assert np.abs(scene.piano.note_range_dynamics.value - first).max() > 1.0


# ---- 3. chunks against batches ---------------------------------------------------------------------------------------------------------

def test_chunks_of_seven_in_batches_of_twenty(monkeypatch):
    from shaderflow_amd.clockloop import ClockLoop
    from shaderflow_amd.tape import FrameTape
    Scene, frames = piano_audio(), 45
    loop, want = frame_loop(Scene, frames, monkeypatch)
    calls = []

    def seven(self, measured):
        calls.append(7)
        return 7
    monkeypatch.setattr(ClockLoop, "chunk_frames", seven)
    monkeypatch.setattr(FrameTape, "BATCH", 20)
    scene = Scene()
    got = render(scene, frames)
    assert scene.piano_tape is not None and scene.piano_tape.frames == frames and scene.piano_tape.tape.tape.batch == 20
    assert len(calls) == 7                                              # 7 7 6 | 7 7 6 | 5: a chunk ends with its batch, never across it
    assert_frames_equal(want, got)
    assert_same_piano(loop, scene)


# ---- 4. a piano under another name ---------------------------------------------------------------------------------------------------------

def renamed_scene():
    """iRoll…: its textures, its uniforms, and what the fragment reads. A note far behind the run makes the note range travel, so a frame
    drawn with another frame's iRollDynamic is another picture"""
    from examples.scenes import PianoAudio, _AudioScene
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    from shaderflow_amd.piano import ShaderPiano

    class Renamed(PianoAudio):
        FRAGMENT = PianoAudio.FRAGMENT.replace("iPiano", "iRoll")
        audio_source = (clip(), 44100)

        def build(self):
            _AudioScene.build(self)
            self.piano = ShaderPiano(scene=self, name="iRoll")
            for note in [*score(), PianoNote(note=100, start=30.0, end=30.5, channel=2, velocity=90)]:
                self.piano.add_note(note)
            self._load_audio()
            self.spectrogram = ShaderSpectrogram(scene=self, length=0, audio=self.audio, smooth=False)
            self.spectrogram.from_notes(start=self.SPECTRUM_LOW, end=self.SPECTRUM_HIGH, piano=True)
            self.shader.fragment = self.FRAGMENT
    return Renamed


def test_a_piano_under_another_name(monkeypatch):
    Scene, frames = renamed_scene(), 75
    loop, want = frame_loop(Scene, frames, monkeypatch)
    scene = Scene()
    got = render(scene, frames)
    assert scene.piano_tape is not None and scene.piano_tape.piano.dynamic_name == b"iRollDynamic"
    assert scene.shader.translated and not scene.shader.fallback
    names = {u.name for u in scene.shader.full_pipeline()}
    assert {"iRollDynamic", "iRollRoll0x0", "iRollKeys0x0"} <= names and "iPianoDynamic" not in names
    assert_frames_equal(want, got)
    first = np.array([scene.piano.global_minimum_note, scene.piano.global_maximum_note], np.float32)
    assert np.abs(scene.piano.note_range_dynamics.value - first).max() > 1.0
    assert np.array_equal(scene.piano.note_range_dynamics.value, loop.piano.note_range_dynamics.value)


# ---- 5. nothing runs on the host -------------------------------------------------------------------------------------------------------

def test_no_update_of_the_piano_or_the_audio_modules_runs(monkeypatch):
    from shaderflow_amd.audio import ShaderAudio
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    from shaderflow_amd.piano import ShaderPiano
    counts = {}
    for cls in (ShaderPiano, ShaderSpectrogram, ShaderAudio):
        def recorder(self, _original=cls.update, _name=cls.__name__):
            counts[_name] = counts.get(_name, 0) + 1
            return _original(self)
        counts[cls.__name__] = 0
        monkeypatch.setattr(cls, "update", recorder)
    scene = piano_audio()()
    render(scene, 75)
    assert scene.piano_tape is not None and scene.piano_tape.frames == 75
    assert counts == {"ShaderPiano": 0, "ShaderSpectrogram": 0, "ShaderAudio": 0}
    loop = piano_audio()()                                              # (the recorders do count: the frame loop calls all three every frame)
    monkeypatch.setenv("SHADERFLOW_PIANO_TAPE", "0")
    monkeypatch.setenv("SHADERFLOW_TAPE_LOOP", "0")
    render(loop, 3)
    assert counts == {"ShaderPiano": 3, "ShaderSpectrogram": 3, "ShaderAudio": 3}


# ---- 6. a run that fails -----------------------------------------------------------------------------------------------------------------

def test_a_run_that_fails_leaves_the_host_objects_at_the_last_frame_drawn(monkeypatch):
    from shaderflow_amd.clockloop import ClockLoop
    from shaderflow_amd.exporting import ExportingHelper
    Scene = piano_audio()
    loop, _ = frame_loop(Scene, 14, monkeypatch)
    monkeypatch.setattr(ClockLoop, "chunk_frames", lambda self, measured: 7)
    calls, check = [], ExportingHelper._check_encoder

    def dies_on_the_third_look(self):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("the encoder went away")
        return check(self)
    monkeypatch.setattr(ExportingHelper, "_check_encoder", dies_on_the_third_look)
    scene = Scene()
    with pytest.raises(RuntimeError, match="encoder went away"):
        scene.main(width=W, height=H, fps=FPS, time=60/FPS, freewheel=True)       # (render-only: no sink is left open behind the failure)
    assert scene.piano_tape is not None and scene.piano_tape.frames == 14
    assert scene.time == loop.time
    assert_same_piano(loop, scene)


# ---- 7. falling back -----------------------------------------------------------------------------------------------------------------------

def fallback_scenes():
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    from shaderflow_amd.piano import ShaderPiano
    from shaderflow_amd.scene import ShaderScene
    PianoAudio = piano_audio()

    class OwnPiano(ShaderPiano):
        pass

    class OwnSpectrogram(ShaderSpectrogram):
        pass

    class Rebuilt(_Parts, ShaderScene):
        """PianoAudio's picture from parts of the test's choosing"""
        piano_kind = spectrogram_kind = None

        def build(self):
            self.piano = self.add_piano(kind=self.piano_kind)
            self.add_audio(kind=self.spectrogram_kind)
            self.shader.fragment = PianoAudio.FRAGMENT

    class SubclassedPiano(Rebuilt):
        piano_kind = OwnPiano

    class SubclassedSpectrogram(Rebuilt):
        spectrogram_kind = OwnSpectrogram

    class TwoPianos(Rebuilt):
        def build(self):
            Rebuilt.build(self)
            self.second = self.add_piano(name="iOther", notes=[PianoNote(note=40, start=0.0, end=1.0)])

    class OwnUpdate(Rebuilt):
        def update(self):
            self.piano.roll_time = 2.0 + 0.5*np.sin(self.time)

    class MovedCamera(Rebuilt):
        def build(self):
            Rebuilt.build(self)
            target = np.array(self.camera.position.target, dtype=np.float64)
            target[-1] += 0.3
            self.camera.position.set(target)                           # at rest, away from the identity pose

    class EarlyOut(Rebuilt):
        def build(self):
            Rebuilt.build(self)
            self.piano.key_press_dynamics.precision = 1e-6

    cases = {name: (Rebuilt, name) for name in SWITCHES}
    cases.update({"subclassed-piano": (SubclassedPiano, None), "two-pianos": (TwoPianos, None), "subclassed-spectrogram": (SubclassedSpectrogram, None),
                  "own-update": (OwnUpdate, None), "moved-camera": (MovedCamera, None), "early-out": (EarlyOut, None)})
    return cases


@pytest.mark.parametrize("case", [*SWITCHES, "subclassed-piano", "two-pianos", "subclassed-spectrogram", "own-update", "moved-camera", "early-out"])
def test_scenes_the_sequence_does_not_take_keep_their_frames(case, monkeypatch):
    Scene, switch = fallback_scenes()[case]
    frames = 40
    _, want = frame_loop(Scene, frames, monkeypatch)
    if switch:
        monkeypatch.setenv(switch, "0")
    scene = Scene()
    got = render(scene, frames)
    assert scene.piano_tape is None
    assert_frames_equal(want, got)
    if switch:                                                          # … and without the switch the same scene is the sequence's
        monkeypatch.delenv(switch)
        scene = Scene()
        assert_frames_equal(want, render(scene, frames))
        assert scene.piano_tape is not None and scene.piano_tape.frames == frames


# ---- 8. the other loops keep their scenes ----------------------------------------------------------------------------------------------------

def test_scenes_of_the_other_loops_keep_them(monkeypatch):
    from examples.scenes import AudioTrails, MotionBlur, PianoRoll, Video, make
    from shaderflow_amd.clockloop import ClockLoop
    taken, run = [], ClockLoop.run

    def spy(self, *args, **kwargs):
        taken.append("ClockLoop")
        return run(self, *args, **kwargs)
    monkeypatch.setattr(ClockLoop, "run", spy)
    frames = 6
    for scene, attribute in ((PianoRoll(), "piano_sequence"), (make(AudioTrails, audio=(clip(), 44100)), "tape_sequence"), (Video(), "video_sequence"),
                             (make(MotionBlur, background=synth.background_image(240, 135, seed=7)), None)):
        render(scene, frames)
        assert scene.piano_tape is None, type(scene).__name__
        kept = {name: getattr(scene, name) is not None for name in ("piano_sequence", "tape_sequence", "video_sequence", "tape_loop")}
        assert kept == {name: name == attribute for name in kept}, type(scene).__name__
        assert taken == (["ClockLoop"] if attribute is None else []), type(scene).__name__


# ---- 9. the descriptor ---------------------------------------------------------------------------------------------------------------------

def test_a_piano_beside_a_tape_of_another_context_is_invalid():
    from examples.scenes import MusicBars, make
    from shaderflow_amd import _native as N
    from shaderflow_amd.tape import FrameTape
    scene = make(MusicBars, audio=(clip(), 44100), device=0)            # `device=`: a context of the scene's own
    scene.main(width=64, height=36, fps=FPS, time=2/FPS, freewheel=True, batch=False)
    other = N.default_context()
    assert scene.context is not other and scene.context.handle.value != other.handle.value
    tape = FrameTape(scene).prepare(4)
    try:
        passes, ticks = (N.SequencePass*1)(), (N.ClockTick*1)()
        sequence = N.Sequence(passes=passes, npasses=1, nmatrices=0, clock=ticks, nframes=1, fd=-1, tape=tape.handle, piano=N.Handle(1),
                              piano_ticks=(N.PianoTick*1)())
        code = N.lib().sfx_sequence_run(other.handle, C.byref(sequence))
        assert code == -1 and code != N.E_UNSUPPORTED                   # SFX_E_INVALID (include/shaderflow_hip.h)
        assert b"another context" in N.lib().sfx_last_error()
        sequence.piano_ticks = None                                     # … and so is a null tick table, in the tape's own context
        assert N.lib().sfx_sequence_run(scene.context.handle, C.byref(sequence)) == -1
    finally:
        tape.release()
        scene.context.synchronize()
