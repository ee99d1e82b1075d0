"""
The video-joined sequence (shaderflow_amd/sequence.py): a video beside audio modules, a piano or both, without python logic, is drawn by ONE
native sequence that names the staged video AND the audio tape and / or the piano, and every frame equals the frame loop's
(`ShaderScene.next`) byte for byte.

The frame loop here is the real one: `SHADERFLOW_VIDEO_JOIN=0` alone would hand a single-program scene of this kind to the tape loop
(tapeloop.py takes it: the video is python logic to it), so the reference runs switch `SHADERFLOW_TAPE_LOOP` off as well and check that
no loop object was left on the scene.

   1. the MusicVideo example against the frame loop: frames, the video's host state and textures, the clock;
   2. one pass that reads the video, iSpectrogram, iWaveform and iAudioVolume, fused and layered: the tape replaces its two sampler slots
      and nothing of the video's; a video that goes by one of the tape's sampler names is refused by the native call;
   3. the layered routes: a main texture with history, a temporal video read at two depths, a child program that reads the video only;
   4. a planar clip from a .y4m file beside audio;
   5. a video beside a piano, and beside a piano and audio;
   6. calls shortened by the video inside the tape's batches, never across one;
   7. a clip that ends before the scene does;
   8. no `update()` of the video, the piano or the audio modules runs;
   9. a reader that raises fails the export with its exception, the host objects at the last frame drawn;
  10. scenes the loop does not take keep their loop and their frames;
  11. the other loops keep their scenes;
  12. the descriptor: `video_join` lifts the refusal and nothing else.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from shaderflow_amd import synth

pytestmark = pytest.mark.gpu

FPS = 60.0
W, H = 160, 90
RW, RH = 64, 36                                                        # the rgb24 clips
PW, PH = 48, 32                                                        # the planar ones: a width that is no multiple of 16 (k_video_frame's short runs)
LOOPS = ("video_join", "video_sequence", "piano_sequence", "piano_tape", "tape_sequence", "tape_loop")
STATE = ("value", "target", "previous", "derivative", "acceleration")
SOUND = {}


def sweep():
    """Three seconds of stereo sweep at 44100, made once"""
    if "sweep" not in SOUND:
        SOUND["sweep"] = synth.sweep_clip(3.0, 44100)
    return SOUND["sweep"]


def score():
    from examples.scenes import demo_score
    return demo_score(3.0)


def score_sound():
    if "score" not in SOUND:
        SOUND["score"] = synth.score_clip(score(), 3.0)
    return SOUND["score"]


def rgb_clip(count, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (count, RH, RW, 3), dtype=np.uint8)


def planar_clip(count, seed=2):
    return np.random.default_rng(seed).integers(0, 256, (count, PW*PH*3//2), dtype=np.uint8)


def render(scene, frames, ssaa=1.0, pixel_format=None, **kwargs):
    raw = scene.main(width=W, height=H, fps=FPS, ssaa=ssaa, subsample=2, time=frames/FPS, output=bytes, pixel_format=pixel_format, **kwargs)
    per_frame = W*H*3//2 if pixel_format == "yuv420p" else W*H*3
    assert len(raw) == frames*per_frame
    return np.frombuffer(raw, np.uint8).reshape(frames, per_frame)


def taken(scene):
    return {name for name in LOOPS if getattr(scene, name) is not None}


def frame_loop(Scene, frames, monkeypatch, **kwargs):
    """(scene, frames) of `Scene` drawn by ShaderScene.next"""
    monkeypatch.setenv("SHADERFLOW_VIDEO_JOIN", "0")
    monkeypatch.setenv("SHADERFLOW_TAPE_LOOP", "0")
    scene = Scene()
    out = render(scene, frames, **kwargs)
    assert taken(scene) == set()
    monkeypatch.delenv("SHADERFLOW_VIDEO_JOIN")
    monkeypatch.delenv("SHADERFLOW_TAPE_LOOP")
    return scene, out


def assert_frames_equal(loop, sequence):
    assert loop.shape == sequence.shape
    for k in range(loop.shape[0]):
        assert np.array_equal(loop[k], sequence[k]), f"frame {k} differs"


def both_ways(Scene, frames, monkeypatch, **kwargs):
    """(frame loop scene, its frames, joined scene, its frames): equal, and the join drew every frame"""
    loop, want = frame_loop(Scene, frames, monkeypatch, **kwargs)
    scene = Scene()
    got = render(scene, frames, **kwargs)
    assert taken(scene) == {"video_join"} and scene.video_join.frames == frames
    assert all(program.translated and not program.fallback for program in scene.video_join.clock.programs if not program.texture.final)
    assert_frames_equal(want, got)
    return loop, want, scene, got


def assert_same_video(loop, scene):
    """`_read`, `_exhausted`, the clock, and every box of the video's matrix on the device and in its host copy"""
    assert (scene.video._read, scene.video._exhausted) == (loop.video._read, loop.video._exhausted)
    assert (scene.time, scene.dt, scene.rdt) == (loop.time, loop.dt, loop.rdt)
    for depth in range(loop.video.texture.temporal):
        a, b = loop.video.texture.get_box(depth), scene.video.texture.get_box(depth)
        assert np.array_equal(a.texture.read(), b.texture.read()), depth
        assert a.data == b.data and a.empty == b.empty, depth


def piano_textures(piano):
    return (piano.keys_texture.texture.read()[0, :, 0].copy(), piano.channel_texture.texture.read()[0, :, 0].copy(), piano.roll_texture.texture.read().copy())


def assert_same_piano(loop, scene):
    """Both DynamicNumbers field by field, the three textures and the roll's host copy"""
    for name in STATE:
        assert np.array_equal(getattr(loop.piano.key_press_dynamics, name), getattr(scene.piano.key_press_dynamics, name)), f"key_press_dynamics.{name}"
        assert np.array_equal(getattr(loop.piano.note_range_dynamics, name), getattr(scene.piano.note_range_dynamics, name)), f"note_range_dynamics.{name}"
    for what, a, b in zip(("iPianoKeys", "iPianoChan", "iPianoRoll"), piano_textures(loop.piano), piano_textures(scene.piano)):
        assert np.array_equal(a, b), what
    assert scene.piano.roll_texture.get_box().data == loop.piano.roll_texture.get_box().data


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------

def music_video(source):
    """The example with a clip and a sound of the test's (`source()`: fresh per scene, iterators are used up)"""
    from examples.scenes import MusicVideo

    class Scene(MusicVideo):
        audio_source = (sweep(), 44100)

        def build(self):
            self.clip = source()
            MusicVideo.build(self)
    return Scene


def joined_scene(source, fragment, audio=True, waveform=False, piano=False, temporal=1, video_temporal=1, child=None, sound=sweep,
                 video_kind=None, spectrogram_kind=None, video_name="iVideo", spectrogram=True):
    """A scene class of one ShaderVideo made from `source()` (its keyword arguments) beside the parts named"""
    from shaderflow_amd.scene import ShaderScene

    class Joined(ShaderScene):
        def build(self):
            from shaderflow_amd.audio import ShaderAudio
            from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
            from shaderflow_amd.audio.waveform import ShaderWaveform
            from shaderflow_amd.piano import ShaderPiano
            from shaderflow_amd.shader import ShaderProgram
            from shaderflow_amd.video import ShaderVideo
            self.video = (video_kind or ShaderVideo)(scene=self, name=video_name, **source())
            if video_temporal > 1:
                self.video.texture.temporal = video_temporal
            if piano:
                self.piano = ShaderPiano(scene=self)
                for note in score():
                    self.piano.add_note(note)
            if audio:
                self.audio = ShaderAudio(scene=self, name="iAudio")
                self.audio.load(samples=sound(), samplerate=44100)
                if spectrogram:
                    self.spectrogram = (spectrogram_kind or ShaderSpectrogram)(scene=self, length=0, audio=self.audio)
                    self.spectrogram.from_notes(start="C2", end="C7", bins=64)
                if waveform:
                    self.waveform = ShaderWaveform(scene=self, audio=self.audio, smooth=False)
            if child is not None:
                self.child = ShaderProgram(scene=self, name="child")
                self.child.fragment = child
            if temporal > 1:
                self.shader.texture.temporal = temporal
            self.shader.fragment = fragment
    return Joined


def array_source(count=80, fps=30.0, seed=1):
    clip = rgb_clip(count, seed)
    return lambda: dict(frames=clip, fps=fps)


LEVEL = """
        vec2 s = texture(iSpectrogram, vec2(0.5, astuv.x)).xy;
        float level = clamp(sqrt(max(0.5*(s.x + s.y), 0.0))/30.0, 0.0, 1.0);
"""

SLOTS = """
    void main() {
        vec3 clip = texture(iVideo, astuv).rgb;""" + LEVEL + """
        vec2 w = texture(iWaveform, vec2(astuv.x, 0.0)).xy;
        float wave = 1.0 - smoothstep(0.0, 0.06, abs(astuv.y - 0.25 - 0.2*w.x));
        vec3 sound = vec3(step(astuv.y, 0.5*level), wave, clamp(iAudioVolume, 0.0, 1.0));
        fragColor = vec4(astuv.y < 0.5 ? mix(clip, sound, 0.7) : clip, 1.0);
    }
"""

TRAILS = """
    void main() {
        vec3 clip = texture(iVideo, astuv).rgb;""" + LEVEL + """
        vec3 now = mix(clip, vec3(level, 0.2*fract(iTime), 1.0 - level), step(astuv.y, 0.4*level + 0.05));
        vec3 before = 0.6*iScreenTexture(1, 0, astuv).rgb + 0.3*iScreenTexture(3, 0, astuv).rgb;
        fragColor = vec4(max(now, before), 1.0);
    }
"""

DEPTHS = """
    void main() {
        vec4 now = texture(iVideo0x0, astuv), first = texture(iVideo2x0, astuv);""" + LEVEL + """
        vec3 colour = vec3(now.r, first.g, 0.5*(now.b + first.b))*(0.6 + 0.4*clamp(iAudioVolume, 0.0, 1.0));
        fragColor = vec4(mix(colour, vec3(level), step(astuv.y, 0.3*level)), 1.0);
    }
"""

CHILD = """
    void main() {
        fragColor = vec4(texture(iVideo, vec2(astuv.x, 1.0 - astuv.y)).bgr, 1.0);
    }
"""

MAIN = """
    void main() {
        fragColor = vec4(texture(child, astuv).rgb*(0.4 + iAudioVolume) + vec3(0.0, 0.0, 0.2*fract(iTime)), 1.0);
    }
"""

PIANO_KEYS = """
        int note = int(floor(astuv.x*128.0));
        float pressed = clamp(texelFetch(iPianoKeys, ivec2(note, 0), 0).x/100.0, 0.0, 1.0);
        vec4 entry = texelFetch(iPianoRoll, ivec2(0, note), 0);
        float inside = step(iPianoDynamic.x/128.0, astuv.x)*step(astuv.x, (iPianoDynamic.y + 1.0)/128.0);
        vec3 keys = vec3(pressed, entry.w/127.0, 0.3*inside);
"""

OVER_PIANO = """
    void main() {
        vec3 clip = texture(iVideo, astuv).rgb;""" + PIANO_KEYS + """
        fragColor = vec4(astuv.y < 0.4 ? keys + 0.3*clip : clip, 1.0);
    }
"""

OVER_PIANO_AND_AUDIO = """
    void main() {
        vec3 clip = texture(iVideo, astuv).rgb;""" + PIANO_KEYS + LEVEL + """
        vec3 colour = astuv.y < 0.4 ? keys*(0.5 + clamp(iAudioVolume, 0.0, 1.0)) + 0.3*clip : clip;
        fragColor = vec4(mix(colour, vec3(level, 1.0 - level, 0.5), step(0.9, astuv.y)*step(astuv.y, 0.9 + 0.1*level)), 1.0);
    }
"""


# ---- 1. the example against the frame loop -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ssaa, pixel_format", [(1.0, "rgb24"), (2.0, "rgb24"), (1.0, "yuv420p")])
def test_music_video_gives_the_frame_loops_bytes(ssaa, pixel_format, monkeypatch):
    clip = rgb_clip(64)
    Scene, frames = music_video(lambda: (clip, 24.0)), 150               # two full tape batches of 60 and a partial one
    loop, want, scene, got = both_ways(Scene, frames, monkeypatch, ssaa=ssaa, pixel_format=pixel_format)
    assert scene.video_join.tape is not None and scene.video_join.piano is None
    assert len({frame.tobytes() for frame in got}) > frames//2          # the picture moves
    assert 58 <= scene.video._read <= 60 and not scene.video._exhausted
    assert_same_video(loop, scene)


def test_the_picture_shows_the_clip_and_the_sound(monkeypatch):
    """The strip along the bottom and the glow come from the audio: the same clip over silence is another picture; another clip under
    the same sound is another picture as well"""
    from examples.scenes import MusicVideo, make
    frames = 40
    clip = rgb_clip(24)
    played = render(music_video(lambda: (clip, 30.0))(), frames)
    silent_scene = make(MusicVideo, audio=(np.zeros_like(sweep()), 44100), clip=(clip, 30.0))
    silent = render(silent_scene, frames)
    other = render(music_video(lambda: (rgb_clip(24, seed=9), 30.0))(), frames)
    assert silent_scene.video_join is not None
    assert not np.array_equal(played[-1], silent[-1]) and not np.array_equal(played[-1], other[-1])


# ---- 2. the sampler slots ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["fused", "layered"])
def test_one_pass_reads_the_video_and_everything_the_tape_replaces(route, monkeypatch):
    # fused: shade and resolve in one kernel, through sfx_render_tape (2x SSAA: final.glsl's taps stay inside the pixel's supersamples);
    # layered: a main texture with a second row, drawn into row 0 through render_box, then resolved
    ssaa, temporal = (2.0, 1) if route == "fused" else (1.0, 2)
    Scene = joined_scene(array_source(), SLOTS, waveform=True, temporal=temporal)
    loop, want, scene, got = both_ways(Scene, 75, monkeypatch, ssaa=ssaa)
    assert scene._can_fuse(scene.shader) == (route == "fused")           # (else a layered pass into row 0, drawn through render_box)
    names = {u.name for u in scene.shader.full_pipeline()}
    assert {"iVideo0x0", "iSpectrogram0x0", "iWaveform0x0", "iAudioVolume"} <= names
    assert len({frame.tobytes() for frame in got}) > 37
    assert_same_video(loop, scene)
    # the video is in the picture (another clip: other frames) and so is the sound (silence: other frames)
    other = render(joined_scene(array_source(seed=5), SLOTS, waveform=True, temporal=temporal)(), 12, ssaa=ssaa)
    quiet = render(joined_scene(array_source(), SLOTS, waveform=True, temporal=temporal, sound=lambda: np.zeros_like(sweep()))(), 12, ssaa=ssaa)
    assert not np.array_equal(other[-1], got[11]) and not np.array_equal(quiet[-1], got[11])


def test_a_video_under_one_of_the_tapes_sampler_names_is_refused_by_the_native_call(monkeypatch):
    """A ShaderVideo called iSpectrogram: the translator gives its sampler slot 1, the slot the tape replaces for a pass that reads audio.
    The host loop never takes such a scene; forced through it, the native call says which sampler instead of drawing the tape's column"""
    from shaderflow_amd import _native as N
    from shaderflow_amd.sequence import Sequence
    fragment = "void main() { fragColor = vec4(texture(iSpectrogram, astuv).rgb*(0.5 + iAudioVolume), 1.0); }"
    Scene = joined_scene(array_source(), fragment, spectrogram=False, video_name="iSpectrogram")
    applicable = Sequence.applicable
    monkeypatch.setattr(Sequence, "applicable", staticmethod(lambda *args, **kwargs: True))
    scene = Scene()
    with pytest.raises(N.NativeError, match="reads the video through sampler iSpectrogram") as raised:
        scene.main(width=W, height=H, fps=FPS, time=8/FPS, freewheel=True)
    assert raised.value.code == -1                                      # SFX_E_INVALID
    assert scene.video_join is not None and scene.video_join.frames == 0
    assert not applicable(scene)                                        # asked, the loop refuses the scene
    named = joined_scene(array_source(), fragment.replace("iSpectrogram", "iClip"), spectrogram=False, video_name="iClip")()
    render(named, 4)
    assert named.video_join is not None                                 # … for its name alone


# ---- 3. the layered routes -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["history", "video-depths", "two-programs"])
def test_layered_temporal_and_multi_program_scenes(case, monkeypatch):
    Scene = {"history": lambda: joined_scene(array_source(), TRAILS, temporal=4),
             "video-depths": lambda: joined_scene(array_source(), DEPTHS, video_temporal=3),
             "two-programs": lambda: joined_scene(array_source(), MAIN, child=CHILD, spectrogram=False)}[case]()
    loop, want, scene, got = both_ways(Scene, 75, monkeypatch)
    assert len({frame.tobytes() for frame in got}) > 37
    assert_same_video(loop, scene)
    if case == "video-depths":
        rows = [scene.video.texture.get_box(depth).texture.read() for depth in range(3)]
        assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])


# ---- 4. a planar clip --------------------------------------------------------------------------------------------------------------------------

def write_y4m(path, planar, fps):
    with open(path, "wb") as file:
        file.write(f"YUV4MPEG2 W{PW} H{PH} F{int(fps)}:1 Ip C420jpeg\n".encode())
        for frame in planar:
            file.write(b"FRAME\n" + frame.tobytes())
    return path


def test_a_y4m_clip_beside_audio(monkeypatch, tmp_path):
    path = write_y4m(tmp_path/"clip.y4m", planar_clip(40), 30.0)
    loop, want, scene, got = both_ways(music_video(lambda: path), 75, monkeypatch)
    assert scene.video.format == "i420" and (scene.video.width, scene.video.height) == (PW, PH)
    assert 36 <= scene.video._read <= 38
    assert_same_video(loop, scene)


# ---- 5. a piano ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("audio", [False, True])
def test_a_video_beside_a_piano(audio, monkeypatch):
    Scene = joined_scene(array_source(), OVER_PIANO_AND_AUDIO if audio else OVER_PIANO, audio=audio, piano=True, sound=score_sound)
    loop, want, scene, got = both_ways(Scene, 75, monkeypatch)
    assert scene.video_join.piano is not None and (scene.video_join.tape is not None) == audio
    assert [type(part).__name__ for part in scene.video_join.parts] == ["PianoSequence", *(["TapeSequence"] if audio else []), "VideoSequence"]
    assert_same_video(loop, scene)
    assert_same_piano(loop, scene)
    assert scene.piano.key_press_dynamics.value.any() and piano_textures(scene.piano)[2].any()


# ---- 6. calls the video shortens, inside the tape's batches ------------------------------------------------------------------------------------

def test_short_calls_stay_inside_the_tapes_batches(monkeypatch):
    from shaderflow_amd import _native as N
    from shaderflow_amd import videosequence
    clip = rgb_clip(70)
    Scene, frames = music_video(lambda: (clip, 30.0)), 130
    loop, want = frame_loop(Scene, frames, monkeypatch)
    monkeypatch.setattr(videosequence, "SLOT_BYTES", 1)
    assert videosequence.slot_count(RW*RH*3) == 4                       # two landings a call
    calls, lib = [], N.lib()
    run = lib.sfx_sequence_run

    def spy(context, reference):
        sequence = reference._obj
        calls.append((int(sequence.tape_frame0), int(sequence.nframes), int(sequence.video_join),
                      sum(1 for i in range(sequence.nframes) if sequence.video_slots[i] >= 0)))
        return run(context, reference)
    monkeypatch.setattr(lib, "sfx_sequence_run", spy)
    scene = Scene()
    got = render(scene, frames)
    monkeypatch.setattr(lib, "sfx_sequence_run", run)
    assert taken(scene) == {"video_join"} and scene.video_join.frames == frames
    batch = scene.video_join.tape.tape.batch
    assert batch == 60 and sum(count for _, count, _, _ in calls) == frames
    first, inside, at_end = 0, 0, 0
    for frame0, count, join, landings in calls:
        size = min(batch, frames - first//batch*batch)
        assert join == 1 and count >= 1 and landings <= 2
        assert frame0 == first % batch                                  # the call starts where the last one ended, inside its batch
        assert frame0 + count <= size, (first, frame0, count)           # … and never crosses the batch's end
        if frame0 + count == size:
            at_end += 1
        else:
            inside += 1
        first += count
    assert at_end == 3 and inside >= 3*at_end                           # 60 + 60 + 10 frames, each batch in calls of about four frames
    assert_frames_equal(want, got)
    assert_same_video(loop, scene)


# ---- 7. a clip that ends early -------------------------------------------------------------------------------------------------------------------

def test_a_clip_that_ends_before_the_scene_holds_its_last_frame(monkeypatch):
    clip = rgb_clip(20)
    loop, want, scene, got = both_ways(music_video(lambda: (clip, 30.0)), 120, monkeypatch)      # 2 s; the clip is over after 0.67 s
    assert scene.video._read == 20 and scene.video._exhausted
    assert_same_video(loop, scene)
    assert np.array_equal(scene.video.texture.get_box().texture.read(), np.flipud(clip[19]))


# ---- 8. nothing runs on the host -----------------------------------------------------------------------------------------------------------------

def test_no_update_of_the_video_the_piano_or_the_audio_modules_runs(monkeypatch):
    from shaderflow_amd.audio import ShaderAudio
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    from shaderflow_amd.piano import ShaderPiano
    from shaderflow_amd.video import ShaderVideo
    Scene = joined_scene(array_source(), OVER_PIANO_AND_AUDIO, piano=True, sound=score_sound)
    _, want = frame_loop(Scene, 30, monkeypatch)
    for cls in (ShaderVideo, ShaderPiano, ShaderSpectrogram, ShaderAudio):
        def raises(self, _name=cls.__name__):
            raise AssertionError(f"{_name}.update() ran on the host")
        monkeypatch.setattr(cls, "update", raises)
    scene = Scene()
    got = render(scene, 30)
    assert taken(scene) == {"video_join"} and scene.video_join.frames == 30
    assert_frames_equal(want, got)


# ---- 9. a reader that raises ---------------------------------------------------------------------------------------------------------------------

def test_a_reader_that_raises_fails_the_export_and_leaves_the_last_frame_drawn(monkeypatch, tmp_path):
    from shaderflow_amd.exporting import ExportingHelper
    from shaderflow_amd.scheduler import freewheel_clock
    from shaderflow_amd.videosequence import landing_frames
    clip, frames = rgb_clip(60), 120

    def decoder():
        for k, frame in enumerate(clip):
            if k == 40:
                raise ValueError("the decoder went away")
            yield frame
    wanted_it = int(np.flatnonzero(landing_frames(freewheel_clock(FPS, frames, 1.0)[0], 30.0) == 40)[0])
    loop, want = frame_loop(music_video(lambda: (clip, 30.0)), wanted_it, monkeypatch)
    exports, popen = [], ExportingHelper.popen

    def remembered(self, *args, **kwargs):
        exports.append(self)
        return popen(self, *args, **kwargs)
    monkeypatch.setattr(ExportingHelper, "popen", remembered)
    scene = failing_scene(decoder)()
    with pytest.raises(ValueError, match="decoder went away"):
        scene.main(width=W, height=H, fps=FPS, subsample=2, time=frames/FPS, output=tmp_path/"out.rgb")
    assert taken(scene) == {"video_join"}
    # as in the frame loop, the exception comes out of the frame that wanted source frame 40: every frame in front of it was drawn
    assert scene.video_join.frames == wanted_it and scene.video._read == 40 and not scene.video._exhausted
    export = exports[-1]
    export.drain()
    export.finish()
    delivered = np.fromfile(tmp_path/"out.rgb", np.uint8)
    assert delivered.size == wanted_it*W*H*3
    assert_frames_equal(want, delivered.reshape(wanted_it, W*H*3))
    assert_same_video(loop, scene)
    assert scene.video_join.tape.tape.handle is None and scene.video_join.video.stage is None      # released, the tape as well
    # a second, ordinary export on a fresh scene
    monkeypatch.setattr(ExportingHelper, "popen", popen)
    again = music_video(lambda: (clip, 30.0))()
    assert_frames_equal(want[:30], render(again, 30))
    assert taken(again) == {"video_join"}


def failing_scene(decoder):
    """MusicVideo over an iterator source, which carries no size of its own"""
    from examples.scenes import MusicVideo
    from shaderflow_amd.video import ShaderVideo

    class Scene(MusicVideo):
        audio_source = (sweep(), 44100)

        def build(self):
            from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
            from shaderflow_amd.piano import PianoNote
            self.video = ShaderVideo(scene=self, frames=decoder(), width=RW, height=RH, fps=30.0)
            self._load_audio()
            self.spectrogram = ShaderSpectrogram(scene=self, length=0, audio=self.audio, smooth=False)
            self.spectrogram.from_notes(start=PianoNote.from_frequency(20), end=PianoNote.from_frequency(14000), piano=True)
            self.shader.fragment = self.FRAGMENT
    return Scene


# ---- 10. falling back ------------------------------------------------------------------------------------------------------------------------------

SWITCHES = ("SHADERFLOW_VIDEO_JOIN", "SHADERFLOW_VIDEO_SEQUENCE", "SHADERFLOW_TAPE_SEQUENCE")


def fallback_scenes():
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    from shaderflow_amd.video import ShaderVideo
    source = array_source(30)
    Plain = joined_scene(source, SLOTS, waveform=True)

    class OwnVideo(ShaderVideo):
        pass

    class OwnSpectrogram(ShaderSpectrogram):
        pass

    class TwoVideos(Plain):
        def build(self):
            Plain.build(self)
            self.other = ShaderVideo(scene=self, name="iOther", frames=rgb_clip(30, seed=4), fps=20.0)

    class OwnUpdate(Plain):
        def update(self):
            pass

    class MovedCamera(Plain):
        def build(self):
            Plain.build(self)
            target = np.array(self.camera.position.target, dtype=np.float64)
            target[-1] += 0.3
            self.camera.position.set(target)                           # at rest, away from the identity pose
    cases = {name: (Plain, name) for name in SWITCHES}
    cases.update({"subclassed-video": (joined_scene(source, SLOTS, waveform=True, video_kind=OwnVideo), None), "two-videos": (TwoVideos, None),
                  "own-update": (OwnUpdate, None), "moved-camera": (MovedCamera, None),
                  "subclassed-spectrogram": (joined_scene(source, SLOTS, waveform=True, spectrogram_kind=OwnSpectrogram), None)})
    return cases


@pytest.mark.parametrize("case", [*SWITCHES, "subclassed-video", "two-videos", "own-update", "moved-camera", "subclassed-spectrogram"])
def test_scenes_the_loop_does_not_take_keep_their_loop_and_their_frames(case, monkeypatch):
    Scene, switch = fallback_scenes()[case]
    frames = 40
    _, want = frame_loop(Scene, frames, monkeypatch)
    if switch:
        monkeypatch.setenv(switch, "0")
    scene = Scene()
    got = render(scene, frames)
    # single-program scenes: what drew them before this loop existed draws them still — the tape loop where it takes the scene (the
    # video, a subclass, an update() are python logic to it), else the frame loop
    assert taken(scene) <= {"tape_loop"}
    assert_frames_equal(want, got)
    if switch:                                                          # … and without the switch the same scene is the join's
        monkeypatch.delenv(switch)
        scene = Scene()
        assert_frames_equal(want, render(scene, frames))
        assert taken(scene) == {"video_join"} and scene.video_join.frames == frames


# ---- 11. the other loops keep their scenes -----------------------------------------------------------------------------------------------------------

def test_scenes_of_the_other_loops_keep_them(monkeypatch):
    from examples.scenes import AudioTrails, MotionBlur, PianoAudio, PianoRoll, Video, make
    from shaderflow_amd.clockloop import ClockLoop
    ran, run = [], ClockLoop.run

    def spy(self, *args, **kwargs):
        ran.append("ClockLoop")
        return run(self, *args, **kwargs)
    monkeypatch.setattr(ClockLoop, "run", spy)
    frames = 6
    for scene, attribute in ((Video(), "video_sequence"), (PianoRoll(), "piano_sequence"),
                             (make(PianoAudio, score=score(), audio=(score_sound(), 44100)), "piano_tape"),
                             (make(AudioTrails, audio=(sweep(), 44100)), "tape_sequence"),
                             (make(MotionBlur, background=synth.background_image(240, 135, seed=7)), None)):
        render(scene, frames)
        assert scene.video_join is None, type(scene).__name__
        assert taken(scene) == ({attribute} if attribute else set()), type(scene).__name__
        assert ran == (["ClockLoop"] if attribute is None else []), type(scene).__name__


# ---- 12. the descriptor ------------------------------------------------------------------------------------------------------------------------------

class Stage:
    """sfx_video_* over one bare RGB8 texture of a context"""

    def __init__(self, context, w=8, h=6):
        from shaderflow_amd import _native as N
        self.lib, self.context, self.texture, self.handle = N.lib(), context, N.Handle(), N.Handle()
        N.check(self.lib.sfx_texture_create(context.handle, w, h, 3, N.U8, C.byref(self.texture)))
        N.check(self.lib.sfx_video_create(context.handle, (N.Handle*1)(self.texture), 1, w, h, N.VIDEO_RGB24, 1, C.byref(self.handle)))

    def close(self):
        self.lib.sfx_video_destroy(self.handle)
        self.lib.sfx_texture_destroy(self.texture)


def test_video_join_lifts_the_refusal_and_no_other_check():
    from shaderflow_amd import _native as N
    stage = Stage(N.default_context())
    lib, context = stage.lib, stage.context.handle
    try:
        slots = (C.c_int32*1)(-1)
        passes, ticks = (N.SequencePass*1)(), (N.ClockTick*1)()

        def descriptor(**fields):
            return N.Sequence(passes=passes, npasses=1, nmatrices=0, clock=ticks, nframes=1, fd=-1, video=stage.handle, video_slots=slots,
                              piano_ticks=(N.PianoTick*1)(), **fields)
        # a bogus handle beside the video. A handle is an address the library reads the object's tag at, so one that gets past the
        # refusal must be readable: a texture's, which is neither a tape nor a piano
        bogus = stage.texture
        for other in ("piano", "tape"):
            # unsupported without the field, as ever; with it the handle checks are reached
            assert lib.sfx_sequence_run(context, C.byref(descriptor(**{other: N.Handle(1)}))) == N.E_UNSUPPORTED
            assert lib.sfx_sequence_run(context, C.byref(descriptor(**{other: bogus, "video_join": 0}))) == N.E_UNSUPPORTED
            assert b"a video together with a tape or a piano" in lib.sfx_last_error()
            code = lib.sfx_sequence_run(context, C.byref(descriptor(**{other: bogus, "video_join": 1})))
            assert code == -1 and code != N.E_UNSUPPORTED                # SFX_E_INVALID (include/shaderflow_hip.h)
        assert b"invalid tape handle" in lib.sfx_last_error()
        joined = descriptor(tape=bogus, video_join=1)
        joined.video_slots = None                                        # a null slot table
        assert lib.sfx_sequence_run(context, C.byref(joined)) == -1 and b"null slot table" in lib.sfx_last_error()
        joined = descriptor(piano=bogus, video_join=1)
        joined.piano_ticks = None                                        # a null tick table
        assert lib.sfx_sequence_run(context, C.byref(joined)) == -1 and b"null tick table" in lib.sfx_last_error()
        # the field alone changes nothing for a video on its own: the pass table is looked at next (no program in it)
        alone = lib.sfx_sequence_run(context, C.byref(descriptor(video_join=1)))
        assert alone == lib.sfx_sequence_run(context, C.byref(descriptor())) == -1
    finally:
        stage.close()


def test_a_video_beside_a_tape_of_another_context_is_invalid():
    from examples.scenes import MusicBars, make
    from shaderflow_amd import _native as N
    from shaderflow_amd.tape import FrameTape
    scene = make(MusicBars, audio=(sweep(), 44100), device=0)           # `device=`: a context of the scene's own
    scene.main(width=64, height=36, fps=FPS, time=2/FPS, freewheel=True, batch=False)
    other = N.default_context()
    assert scene.context is not other and scene.context.handle.value != other.handle.value
    tape = FrameTape(scene).prepare(4)
    mine, theirs = Stage(other), Stage(scene.context)
    try:
        slots = (C.c_int32*1)(-1)
        passes, ticks = (N.SequencePass*1)(), (N.ClockTick*1)()
        sequence = N.Sequence(passes=passes, npasses=1, nmatrices=0, clock=ticks, nframes=1, fd=-1, tape=tape.handle, video=mine.handle,
                              video_slots=slots, video_join=1)
        assert N.lib().sfx_sequence_run(other.handle, C.byref(sequence)) == -1
        assert b"the tape belongs to another context" in N.lib().sfx_last_error()
        sequence.video = theirs.handle                                   # … and a video of another context, in front of the tape's check
        assert N.lib().sfx_sequence_run(other.handle, C.byref(sequence)) == -1
        assert b"invalid video handle, or one of another context" in N.lib().sfx_last_error()
        sequence.tape_frame0 = 1 << 20                                         # frames outside the tape, everything in the tape's own context
        assert N.lib().sfx_sequence_run(scene.context.handle, C.byref(sequence)) == -1
        assert b"outside the tape" in N.lib().sfx_last_error()
    finally:
        mine.close()
        theirs.close()
        tape.release()
        scene.context.synchronize()
