"""
The piano sequence (shaderflow_amd/pianosequence.py, csrc/piano_kernels.hpp k_piano_frame): the score on the device, each frame's
iPianoKeys / iPianoChan / iPianoRoll made by one kernel launch, the frames of an export drawn by the native sequence.

  1. the kernel, stepped frame by frame, against the reference's own values (tests/golden/piano.npz), bit for bit;
  2. edge scores against the host module (`ShaderPiano.update()`), bit for bit per frame — each score is first checked, through the
     host module, to really produce the case it is there for;
  3. the export of the PianoRoll example equals the frame loop's (`SHADERFLOW_PIANO_SEQUENCE=0`) byte for byte;
  4. scenes the sequence does not take keep the frame loop and their frames;
  5. the PianoRoll picture shows the score.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from shaderflow_amd.piano import PianoNote
from shaderflow_amd.piano.module import MAX_NOTE, MAX_ROLLING

pytestmark = pytest.mark.gpu

GOLDEN = np.load(Path(__file__).parent/"golden"/"piano.npz")
FPS = 60.0
W, H = 160, 90
STATE = ("value", "target", "previous", "derivative", "acceleration")


def golden_score():
    return [PianoNote(note=int(n), start=float(s), end=float(e), channel=int(c), velocity=int(v)) for n, s, e, c, v in GOLDEN["notes"]]


def piano_scene(score, **fields):
    """An initialised PianoRoll scene with `score`, ShaderPiano fields set from `fields`"""
    from examples.scenes import PianoRoll, make
    scene = make(PianoRoll, score=list(score))
    scene.initialize()
    for name, value in fields.items():
        setattr(scene.piano, name, value)
    return scene


def textures(piano):
    """(keys (128,), channels (128,), roll (128, 256, 4)) as the device holds them"""
    return (piano.keys_texture.texture.read()[0, :, 0].copy(), piano.channel_texture.texture.read()[0, :, 0].copy(),
            piano.roll_texture.texture.read().copy())


def clock(frames, fps=FPS, speed=1.0):
    from shaderflow_amd.scheduler import freewheel_clock
    times, dts, _ = freewheel_clock(fps, frames, speed)
    return times, dts


def host_frames(score, times, dts, **fields):
    """ShaderPiano.update() frame by frame on a scene of its own: per frame (keys, channels, roll, key target), and the module"""
    scene = piano_scene(score, **fields)
    piano, out = scene.piano, []
    for time, dt in zip(times, dts):
        scene.time, scene.dt = time, dt
        piano.update()
        out.append((*textures(piano), piano.key_press_dynamics.target.copy()))
    return out, piano


def device_frames(score, times, dts, **fields):
    """The same frames from sfx_piano_step, and the module after sfx_piano_state_read and the host-stepped note range"""
    from shaderflow_amd.pianosequence import PianoSequence, step_note_range
    scene = piano_scene(score, **fields)
    sequence, out = PianoSequence(scene), []
    sequence.upload()
    try:
        for time, dt in zip(times, dts):
            sequence.step(time, dt)
            out.append(textures(scene.piano))
        sequence.read_state()
    finally:
        sequence.release()
    dynamic = step_note_range(scene.piano, times, dts)
    return out, scene.piano, dynamic


def assert_same_frames(score, times, dts, **fields):
    want, host = host_frames(score, times, dts, **fields)
    got, device, _ = device_frames(score, times, dts, **fields)
    for k, (a, b) in enumerate(zip(want, got)):
        assert np.array_equal(a[0], b[0]), f"iPianoKeys of frame {k}"
        assert np.array_equal(a[1], b[1]), f"iPianoChan of frame {k}"
        assert np.array_equal(a[2], b[2]), f"iPianoRoll of frame {k}"
    for name in STATE:
        assert np.array_equal(getattr(host.key_press_dynamics, name), getattr(device.key_press_dynamics, name)), f"key_press_dynamics.{name}"
        assert np.array_equal(getattr(host.note_range_dynamics, name), getattr(device.note_range_dynamics, name)), f"note_range_dynamics.{name}"
    assert (host.key_press_dynamics.previous is host.key_press_dynamics.target) == (device.key_press_dynamics.previous is device.key_press_dynamics.target)
    return want


# ---- 1. the kernel against the reference's own values ---------------------------------------------------------------------------------

def test_kernel_matches_the_reference_frame_by_frame():
    fps, frames = float(GOLDEN["fps"]), int(GOLDEN["frames"])
    times, dts, time, dt = [], [], 0.0, 0.0
    for _ in range(frames):                                            # the fixture's clock: time += 1/fps, first dt = 0
        times.append(time); dts.append(dt)
        dt = 1.0/fps
        time += dt
    got, piano, dynamic = device_frames(golden_score(), times, dts)
    assert (piano.global_minimum_note, piano.global_maximum_note) == (int(GOLDEN["global_min"]), int(GOLDEN["global_max"]))
    index, rows = GOLDEN["roll_index"], GOLDEN["roll_rows"]
    for k, (keys, channels, roll) in enumerate(got):
        assert np.array_equal(keys, GOLDEN["keys"][k]), k
        assert np.array_equal(channels, GOLDEN["channels"][k]), k
        assert np.array_equal(dynamic[k], GOLDEN["dynamic"][k]), k
        want = np.zeros((MAX_NOTE, MAX_ROLLING, 4), np.float32)
        part = rows[index[k]:index[k + 1]]
        want[part[:, 0].astype(int), part[:, 1].astype(int)] = part[:, 2:]
        assert roll.dtype == np.float32 and np.array_equal(roll, want), k
    assert np.array_equal(piano.key_press_dynamics.value, GOLDEN["keys"][-1])


# ---- 2. edge scores against the host module ------------------------------------------------------------------------------------------

def frame_at(times, when):
    return int(np.argmin(np.abs(np.asarray(times) - when)))


def test_overlapping_notes_of_one_pitch_on_different_channels():
    times, dts = clock(150)
    first, second = PianoNote(note=60, start=0.2, end=1.5, channel=1, velocity=50), PianoNote(note=60, start=0.6, end=1.0, channel=2, velocity=90)
    # a third one inserted BEFORE a note that has begun earlier: insertion order, not start order, decides among begun notes
    third, fourth = PianoNote(note=72, start=0.9, end=1.4, channel=4, velocity=30), PianoNote(note=72, start=0.4, end=1.4, channel=5, velocity=99)
    want = assert_same_frames([first, second, third, fourth], times, dts)
    keys, channels, roll, target = want[frame_at(times, 0.8)]          # both of pitch 60 sound
    assert roll[60, 0].tolist() == [np.float32(0.2), np.float32(1.5), 1.0, 50.0] and roll[60, 1, 2] == 2.0 and not roll[60, 2:].any()
    assert channels[60] == 2.0 and target[60] == 90.0                   # the later one in the visiting order wins
    keys, channels, roll, target = want[frame_at(times, 1.2)]
    assert channels[60] == 1.0 and target[60] == 50.0                   # … and the first one takes over again when it ends
    assert channels[72] == 5.0 and target[72] == 99.0 and roll[72, 0, 2] == 4.0 and roll[72, 1, 2] == 5.0


def test_note_shorter_than_release_before_end():
    times, dts = clock(120)
    inside = times[30]
    short = PianoNote(note=64, start=inside - 0.004, end=inside + 0.016, channel=3, velocity=77)          # 0.02 s < release_before_end
    usual = PianoNote(note=65, start=inside - 0.5, end=inside + 0.016, channel=0, velocity=66)            # inside its last 0.03 s
    want = assert_same_frames([short, usual], times, dts, release_before_end=0.03)
    keys, channels, roll, target = want[30]
    assert channels[64] == 3.0 and target[64] == 77.0                   # pressed although time >= end - release_before_end
    assert channels[65] == 0.0 and target[65] == 0.0                    # an ordinary note is released there, still playing
    assert want[33][0][64] > 0.0                                        # the key moved


def test_note_that_ended_earlier_in_the_current_second():
    times, dts = clock(150)
    ended = PianoNote(note=50, start=1.1, end=1.2, channel=2, velocity=80)
    later = PianoNote(note=50, start=3.0, end=3.5, channel=1, velocity=81)
    want = assert_same_frames([later, ended], times, dts)
    keys, channels, roll, target = want[frame_at(times, 1.6)]
    assert roll[50, 0].tolist() == [np.float32(1.1), np.float32(1.2), 2.0, 80.0]       # still a candidate of second 1, in slot 0
    assert roll[50, 1, 2] == 1.0 and channels[50] == -1.0 and target[50] == 0.0
    assert want[frame_at(times, 2.05)][2][50, 0, 2] == 1.0                          # gone with its second


def test_note_that_starts_exactly_at_the_edge_of_the_roll():
    times, dts = clock(120)
    roll_time = 2.0
    edge = PianoNote(note=70, start=times[20] + roll_time, end=times[20] + roll_time + 0.5, channel=1, velocity=60)
    want = assert_same_frames([edge], times, dts, roll_time=roll_time)
    assert not want[20][2][70].any()                                    # start < time + roll_time is false at equality
    assert want[21][2][70, 0, 3] == 60.0


def test_more_than_256_visible_notes_on_one_pitch():
    times, dts = clock(120)
    crowd = [PianoNote(note=64, start=0.5 + 0.001*k, end=2.5, channel=k % 7, velocity=1 + k % 120) for k in range(300)]
    crowd += [PianoNote(note=65, start=0.25*k, end=0.25*k + 0.2, channel=1, velocity=100) for k in range(8)]
    want = assert_same_frames(crowd, times, dts)
    keys, channels, roll, target = want[frame_at(times, 1.5)]           # all 300 sound
    assert roll[64, 255, 2] == 255 % 7 and roll[64, 255, 3] == 1 + 255 % 120 and roll[64, :, 1].all()
    assert channels[64] == 299 % 7 and target[64] == 1 + 299 % 120      # the last candidate decides, although its slot was dropped
    assert 299 % 7 != 255 % 7


def test_empty_score():
    times, dts = clock(40)
    want = assert_same_frames([], times, dts)
    assert not want[-1][2].any() and (want[-1][1] == -1.0).all()


def test_time_offset():
    times, dts = clock(150)
    offset = -0.73
    score = [PianoNote(note=55, start=0.1, end=0.6, channel=1, velocity=70), PianoNote(note=57, start=0.9, end=1.6, channel=2, velocity=80)]
    want = assert_same_frames(score, times, dts, time_offset=offset, roll_time=1.5, lookahead=1.25)
    plain, _ = host_frames(score, times, dts, roll_time=1.5, lookahead=1.25)
    k = frame_at(times, 1.0)                                           # the module's time there is 0.27: the first note sounds, not the second
    assert want[k][1][55] == 1.0 and want[k][3][55] == 70.0 and want[k][1][57] == -1.0
    assert plain[k][1][55] == -1.0 and plain[k][1][57] == 2.0 and plain[k][3][57] == 80.0       # … and without the offset it is the other way round
    assert not np.array_equal(want[k][2], plain[k][2])
    assert_same_frames(golden_score(), times, dts, time_offset=0.31)


def test_speed():
    speed, fps = 1.7, 50.0
    times, dts = clock(150, fps=fps, speed=speed)
    unhurried, _ = clock(150, fps=fps)
    assert dts[0] == 0.0 and dts[1] == pytest.approx(speed/fps) and times[100] == pytest.approx(speed*unhurried[100])
    score = [PianoNote(note=62, start=3.0, end=3.3, channel=3, velocity=90)]
    want = assert_same_frames(score, times, dts)
    slow, _ = host_frames(score, unhurried, [abs(dt)/speed for dt in dts])
    k = frame_at(times, 3.1)                                           # frame k is at 3.1 s of the score at this speed, at 1.8 s without it
    assert want[k][1][62] == 3.0 and want[k][3][62] == 90.0 and slow[k][1][62] == -1.0
    assert want[k + 2][0][62] > 0.0 and slow[k + 2][0][62] == 0.0        # the key moves here, and has not been touched there
    assert_same_frames(golden_score(), times, dts)


# ---- 3. the export -------------------------------------------------------------------------------------------------------------------

def render(scene, frames, ssaa=1.0, pixel_format=None, **kwargs):
    raw = scene.main(width=W, height=H, fps=FPS, ssaa=ssaa, subsample=2, time=frames/FPS, output=bytes, pixel_format=pixel_format, **kwargs)
    per_frame = W*H*3//2 if pixel_format == "yuv420p" else W*H*3
    assert len(raw) == frames*per_frame
    return np.frombuffer(raw, np.uint8).reshape(frames, per_frame)


def assert_frames_equal(loop, sequence):
    assert loop.shape == sequence.shape
    for k in range(loop.shape[0]):
        assert np.array_equal(loop[k], sequence[k]), f"frame {k} differs"


@pytest.mark.parametrize("pixel_format", ["rgb24", "yuv420p"])
@pytest.mark.parametrize("ssaa", [1.0, 2.0])
def test_piano_sequence_gives_the_frame_loops_bytes(ssaa, pixel_format, monkeypatch):
    from examples.scenes import PianoRoll
    frames = 96                                                        # chunks of the native call: 30 frames, then what fits a quarter second
    monkeypatch.setenv("SHADERFLOW_PIANO_SEQUENCE", "0")
    loop = PianoRoll()
    want = render(loop, frames, ssaa=ssaa, pixel_format=pixel_format)
    assert loop.piano_sequence is None
    monkeypatch.setenv("SHADERFLOW_PIANO_SEQUENCE", "1")
    scene = PianoRoll()
    got = render(scene, frames, ssaa=ssaa, pixel_format=pixel_format)
    assert scene.piano_sequence is not None and scene.piano_sequence.frames == frames
    assert scene.shader.translated and not scene.shader.fallback
    assert_frames_equal(want, got)
    assert len({frame.tobytes() for frame in got}) > frames//2         # the picture moves
    assert (scene.time, scene.dt, scene.rdt) == (loop.time, loop.dt, loop.rdt)
    for name in STATE:
        assert np.array_equal(getattr(loop.piano.key_press_dynamics, name), getattr(scene.piano.key_press_dynamics, name)), name
        assert np.array_equal(getattr(loop.piano.note_range_dynamics, name), getattr(scene.piano.note_range_dynamics, name)), name
    assert scene.piano.key_press_dynamics.value.any() and scene.piano.note_range_dynamics.value.dtype == np.float32
    for a, b in zip(textures(loop.piano), textures(scene.piano)):
        assert np.array_equal(a, b)
    assert textures(scene.piano)[2].any()
    # the host copy of each texture's last full write follows the device
    assert scene.piano.roll_texture.get_box().data == loop.piano.roll_texture.get_box().data


def test_chunks_of_seven_frames(monkeypatch):
    from examples.scenes import PianoRoll
    from shaderflow_amd.clockloop import ClockLoop
    monkeypatch.setenv("SHADERFLOW_PIANO_SEQUENCE", "0")
    want = render(PianoRoll(), 45)
    monkeypatch.setenv("SHADERFLOW_PIANO_SEQUENCE", "1")
    monkeypatch.setattr(ClockLoop, "chunk_frames", lambda self, measured: 7)
    scene = PianoRoll()
    got = render(scene, 45)
    assert scene.piano_sequence is not None
    assert_frames_equal(want, got)


def renamed_scene():
    """One piano under another name: its textures and uniforms are iRoll…, and so is what the fragment reads. A late high note makes the
    note range travel, so a frame drawn with another frame's iRollDynamic is another picture."""
    from examples.scenes import PianoRoll, demo_score
    from shaderflow_amd.piano import ShaderPiano
    from shaderflow_amd.scene import ShaderScene

    class Renamed(PianoRoll):
        FRAGMENT = PianoRoll.FRAGMENT.replace("iPiano", "iRoll")

        def build(self):
            ShaderScene.build(self)
            self.piano = ShaderPiano(scene=self, name="iRoll")
            for note in [*demo_score(), PianoNote(note=100, start=7.5, end=7.9, channel=2, velocity=90)]:
                self.piano.add_note(note)
            self.shader.fragment = self.FRAGMENT
    return Renamed


def test_a_piano_under_another_name(monkeypatch):
    Scene = renamed_scene()
    frames = 96
    monkeypatch.setenv("SHADERFLOW_PIANO_SEQUENCE", "0")
    loop = Scene()
    want = render(loop, frames)
    monkeypatch.setenv("SHADERFLOW_PIANO_SEQUENCE", "1")
    scene = Scene()
    got = render(scene, frames)
    assert scene.piano_sequence is not None and scene.piano_sequence.piano.dynamic_name == b"iRollDynamic"
    assert scene.shader.translated and not scene.shader.fallback
    names = {u.name for u in scene.shader.full_pipeline()}
    assert {"iRollDynamic", "iRollRoll0x0", "iRollKeys0x0"} <= names and "iPianoDynamic" not in names
    assert_frames_equal(want, got)
    # the note range did travel during the export: the frames depend on each frame's own value
    first = np.array([scene.piano.global_minimum_note, scene.piano.global_maximum_note], np.float32)
    assert np.abs(scene.piano.note_range_dynamics.value - first).max() > 1.0
    assert np.array_equal(scene.piano.note_range_dynamics.value, loop.piano.note_range_dynamics.value)


def test_a_run_that_fails_leaves_the_host_objects_at_the_last_frame_drawn(monkeypatch):
    from examples.scenes import PianoRoll
    from shaderflow_amd.clockloop import ClockLoop
    from shaderflow_amd.exporting import ExportingHelper
    monkeypatch.setenv("SHADERFLOW_PIANO_SEQUENCE", "0")
    loop = PianoRoll()
    render(loop, 14)
    monkeypatch.setenv("SHADERFLOW_PIANO_SEQUENCE", "1")
    monkeypatch.setattr(ClockLoop, "chunk_frames", lambda self, measured: 7)
    calls, check = [], ExportingHelper._check_encoder

    def dies_on_the_third_look(self):
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("the encoder went away")
        return check(self)
    monkeypatch.setattr(ExportingHelper, "_check_encoder", dies_on_the_third_look)
    scene = PianoRoll()
    with pytest.raises(RuntimeError, match="encoder went away"):
        scene.main(width=W, height=H, fps=FPS, time=60/FPS, freewheel=True)       # (render-only: no sink is left open behind the failure)
    assert scene.piano_sequence is not None and scene.piano_sequence.frames == 14
    for name in STATE:
        assert np.array_equal(getattr(loop.piano.key_press_dynamics, name), getattr(scene.piano.key_press_dynamics, name)), name
        assert np.array_equal(getattr(loop.piano.note_range_dynamics, name), getattr(scene.piano.note_range_dynamics, name)), name
    assert scene.time == loop.time
    for a, b in zip(textures(loop.piano), textures(scene.piano)):
        assert np.array_equal(a, b)


# ---- 4. falling back -----------------------------------------------------------------------------------------------------------------

def fallback_scenes():
    from examples.scenes import PianoRoll, demo_score
    from shaderflow_amd.piano import ShaderPiano

    class OwnPiano(ShaderPiano):
        pass

    class Subclassed(PianoRoll):
        def build(self):
            from shaderflow_amd.scene import ShaderScene
            ShaderScene.build(self)
            self.piano = OwnPiano(scene=self)
            for note in demo_score():
                self.piano.add_note(note)
            self.shader.fragment = self.FRAGMENT

    class OwnUpdate(PianoRoll):
        def update(self):
            self.piano.roll_time = 2.0 + 0.5*np.sin(self.time)

    class TwoPianos(PianoRoll):
        def build(self):
            PianoRoll.build(self)
            self.second = ShaderPiano(scene=self, name="iOther")
            self.second.add_note(PianoNote(note=40, start=0.0, end=1.0))

    class WithAudio(PianoRoll):
        def build(self):
            from shaderflow_amd import synth
            from shaderflow_amd.audio import ShaderAudio
            PianoRoll.build(self)
            self.audio = ShaderAudio(scene=self, name="iAudio")
            self.audio.load(samples=synth.sweep_clip(2.0, 44100), samplerate=44100)

    return {"subclass": Subclassed, "own-update": OwnUpdate, "two-pianos": TwoPianos, "audio": WithAudio}


@pytest.mark.parametrize("case", ["subclass", "own-update", "two-pianos", "audio"])
def test_scenes_the_sequence_does_not_take_keep_the_frame_loop(case, monkeypatch):
    Scene = fallback_scenes()[case]
    monkeypatch.setenv("SHADERFLOW_PIANO_SEQUENCE", "0")
    want = render(Scene(), 40)
    monkeypatch.setenv("SHADERFLOW_PIANO_SEQUENCE", "1")
    scene = Scene()
    got = render(scene, 40)
    assert scene.piano_sequence is None
    assert_frames_equal(want, got)
    assert scene.piano.roll_texture.texture.read().any()               # the host module wrote its textures


def test_key_press_system_with_an_early_out_keeps_the_frame_loop():
    from examples.scenes import PianoRoll
    scene = PianoRoll()
    scene.initialize()
    scene.piano.key_press_dynamics.precision = 1e-6
    render(scene, 10)
    assert scene.piano_sequence is None


# ---- 5. the picture ------------------------------------------------------------------------------------------------------------------

def test_the_picture_shows_the_score():
    from examples.scenes import PianoRoll, make
    frames = 70
    scene = PianoRoll()
    played = render(scene, frames)
    assert scene.piano_sequence is not None and scene.shader.translated and not scene.shader.fallback
    silent_scene = make(PianoRoll, score=[])
    silent = render(silent_scene, frames)
    assert silent_scene.shader.translated
    k = frames - 1                                                     # a little past one second: the bass note and a chord note sound
    assert scene.piano.channel_texture.texture.read().max() >= 0
    picture, empty = played[k].reshape(H, W, 3), silent[k].reshape(H, W, 3)      # rows bottom-up
    strip = int(scene.piano.height*H)
    assert not np.array_equal(picture[:strip - 1], empty[:strip - 1])             # the keyboard strip
    assert not np.array_equal(picture[strip + 1:], empty[strip + 1:])             # the roll
    # falling notes: the roll area changes from frame to frame, and holds more than one colour
    assert not np.array_equal(played[k].reshape(H, W, 3)[strip + 1:], played[k - 20].reshape(H, W, 3)[strip + 1:])
    assert len(np.unique(picture[strip + 1:].reshape(-1, 3), axis=0)) > 3
