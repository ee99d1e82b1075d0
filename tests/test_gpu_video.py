"""
The video sequence (shaderflow_amd/videosequence.py, csrc/video_kernels.hpp k_video_frame, csrc/capi_video.hip):

  1. the kernel through sfx_video_step, then sfx_texture_read: rgb24 is np.flipud, I420 is the numpy restatement below of the integer
     BT.601 conversion the header defines (this project's own definition: unpinned against swscale) — bit for bit; the slot protocol's
     refusals through return codes;
  2. the export of video scenes equals the frame loop's (`SHADERFLOW_VIDEO_SEQUENCE=0`) byte for byte: outputs, SSAA, clip rates, every
     kind of source, a temporal matrix, a clip shorter than the scene, chunks of seven frames;
  3. the host objects behind a finished run and behind one cut short, and the frame a further update() shows;
  4. a reader that raises fails the export with its exception;
  5. scenes the sequence does not take keep the frame loop and their frames.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FPS = 60.0
W, H = 96, 54
CW, CH = 32, 18                                                        # the clips' extents


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------

def i420_to_rgb(frame: np.ndarray, w: int, h: int) -> np.ndarray:
    """(h, w, 3) uint8, top row first, of one planar frame: BT.601 limited range in integer arithmetic (arithmetic shifts of signed 32-bit
    values), chroma replicated over its 2 x 2 block — include/shaderflow_hip.h's formulas restated"""
    frame = np.asarray(frame, np.uint8)
    y = frame[:w*h].reshape(h, w).astype(np.int32)
    u = frame[w*h:w*h + (w//2)*(h//2)].reshape(h//2, w//2).astype(np.int32).repeat(2, axis=0).repeat(2, axis=1)
    v = frame[w*h + (w//2)*(h//2):].reshape(h//2, w//2).astype(np.int32).repeat(2, axis=0).repeat(2, axis=1)
    c, d, e = y - 16, u - 128, v - 128
    r = (298*c + 409*e + 128) >> 8
    g = (298*c - 100*d - 208*e + 128) >> 8
    b = (298*c + 516*d + 128) >> 8
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


class Stage:
    """sfx_video_* over `temporal` bare RGB8 textures of the default context"""

    def __init__(self, w, h, planar, temporal=1, slots=1):
        from shaderflow_amd import _native as N
        self.N, self.lib, self.w, self.h = N, N.lib(), w, h
        self.context = N.default_context()
        self.textures = []
        for _ in range(temporal):
            handle = N.Handle()
            N.check(self.lib.sfx_texture_create(self.context.handle, w, h, 3, N.U8, C.byref(handle)))
            self.textures.append(handle)
        self.handle = N.Handle()
        boxes = (N.Handle*temporal)(*self.textures)
        N.check(self.lib.sfx_video_create(self.context.handle, boxes, temporal, w, h, N.VIDEO_I420 if planar else N.VIDEO_RGB24, slots, C.byref(self.handle)))

    def view(self, slot=0):
        pointer, nbytes = C.c_void_p(), C.c_size_t()
        self.N.check(self.lib.sfx_video_slot(self.handle, slot, C.byref(pointer), C.byref(nbytes)))
        return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint8)), shape=(nbytes.value,))

    def show(self, frame, slot=0):
        np.copyto(self.view(slot), np.asarray(frame, np.uint8).reshape(-1))
        self.N.check(self.lib.sfx_video_submit(self.handle, slot))
        self.N.check(self.lib.sfx_video_step(self.handle, slot))

    def read(self, index=0):
        out = np.empty((self.h, self.w, 3), np.uint8)
        self.N.check(self.lib.sfx_texture_read(self.textures[index], out.ctypes.data, out.nbytes))
        return out

    def close(self):
        self.lib.sfx_video_destroy(self.handle)
        for texture in self.textures:
            self.lib.sfx_texture_destroy(texture)


RGB_SIZES = [(2, 2), (64, 36), (1920, 1080), (3840, 2160), (66, 38), (1918, 1078), (65, 37), (1, 1)]
I420_SIZES = [(2, 2), (64, 36), (1920, 1080), (3840, 2160), (66, 38), (1918, 1078)]


@pytest.mark.parametrize("w, h", RGB_SIZES)
def test_rgb24_frames_are_flipped_rows(w, h):
    rng = np.random.default_rng(w*h)
    stage = Stage(w, h, planar=False)
    try:
        for frame in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8),
                      rng.integers(0, 256, (h, w, 3), dtype=np.uint8)):
            stage.show(frame)
            assert np.array_equal(stage.read(), np.flipud(frame))
    finally:
        stage.close()


@pytest.mark.parametrize("w, h", I420_SIZES)
def test_i420_frames_are_the_integer_conversion(w, h):
    rng = np.random.default_rng(w + h)
    n, q = w*h, (w//2)*(h//2)
    random = lambda: rng.integers(0, 256, n + 2*q, dtype=np.uint8)                 # noqa: E731
    frames = [random(), random()]
    for luma, cb, cr in [(0, 0, 0), (255, 255, 255), (0, 255, 0), (255, 0, 255), (255, 0, 0), (0, 0, 255), (16, 128, 128), (235, 128, 128)]:
        frames.append(np.concatenate([np.full(n, luma, np.uint8), np.full(q, cb, np.uint8), np.full(q, cr, np.uint8)]))
    mixed = random()                                                     # random luma over constant extreme chroma planes: both clips per pixel
    mixed[n:n + q], mixed[n + q:] = 255, 0
    frames.append(mixed)
    stage = Stage(w, h, planar=True)
    try:
        clipped = 0
        for frame in frames:
            stage.show(frame)
            want = i420_to_rgb(frame, w, h)
            got = stage.read()
            assert np.array_equal(got, np.flipud(want))
            clipped += int(((want == 0) | (want == 255)).sum())
        assert clipped > 0                                               # the clipping was exercised
    finally:
        stage.close()


def test_a_temporal_matrix_rolls_once_per_frame():
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (5, 6, 8, 3), dtype=np.uint8)
    stage = Stage(8, 6, planar=False, temporal=3, slots=2)
    try:
        for k, frame in enumerate(frames):
            stage.show(frame, slot=k % 2)
        # create order [0, 1, 2]: frame k is written into the box that was oldest: 2, 1, 0, 2, 1
        assert np.array_equal(stage.read(1), np.flipud(frames[4])) and np.array_equal(stage.read(2), np.flipud(frames[3]))
        assert np.array_equal(stage.read(0), np.flipud(frames[2]))
    finally:
        stage.close()


def test_the_slot_protocol_refuses_by_return_code():
    from shaderflow_amd import _native as N
    stage = Stage(8, 6, planar=True, slots=2)
    lib = stage.lib
    try:
        assert lib.sfx_video_step(stage.handle, 0) != N.OK                # nothing submitted
        stage.view(0)[:] = 7
        assert lib.sfx_video_submit(stage.handle, 0) == N.OK
        assert lib.sfx_video_submit(stage.handle, 0) != N.OK              # submitted, not consumed
        assert lib.sfx_video_slot(stage.handle, 0, None, None) != N.OK
        assert lib.sfx_video_step(stage.handle, 0) == N.OK
        assert lib.sfx_video_slot(stage.handle, 0, None, None) == N.OK    # free behind the kernel
        assert lib.sfx_video_submit(stage.handle, 2) != N.OK and lib.sfx_video_step(stage.handle, -1) != N.OK
        assert lib.sfx_video_step(N.Handle(0), 0) != N.OK
        handle = N.Handle()
        boxes = (N.Handle*1)(stage.textures[0])
        assert lib.sfx_video_create(stage.context.handle, boxes, 1, 9, 6, N.VIDEO_I420, 1, C.byref(handle)) != N.OK      # odd extent
        assert lib.sfx_video_create(stage.context.handle, boxes, 1, 8, 8, N.VIDEO_RGB24, 1, C.byref(handle)) != N.OK     # not the texture's size
        assert lib.sfx_video_create(stage.context.handle, boxes, 1, 8, 6, 2, 1, C.byref(handle)) != N.OK                 # no such format
    finally:
        stage.close()


def test_a_video_beside_a_piano_or_a_tape_is_refused():
    from shaderflow_amd import _native as N
    stage = Stage(8, 6, planar=False)
    try:
        slots = (C.c_int32*1)(-1)
        passes, ticks = (N.SequencePass*1)(), (N.ClockTick*1)()
        for other in ("piano", "tape"):
            sequence = N.Sequence(passes=passes, npasses=1, nmatrices=0, clock=ticks, nframes=1, fd=-1, video=stage.handle, video_slots=slots)
            setattr(sequence, other, N.Handle(1))
            sequence.piano_ticks = (N.PianoTick*1)()
            assert stage.lib.sfx_sequence_run(stage.context.handle, C.byref(sequence)) == N.E_UNSUPPORTED
    finally:
        stage.close()


# ---- 2. the sequence against the frame loop -------------------------------------------------------------------------------------------

def rgb_clip(count, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (count, CH, CW, 3), dtype=np.uint8)


def planar_clip(count, seed=2):
    return np.random.default_rng(seed).integers(0, 256, (count, CW*CH*3//2), dtype=np.uint8)


TEMPORAL_FRAGMENT = """
    void main() {
        vec4 now = texture(iVideo0x0, astuv), before = texture(iVideo1x0, astuv), first = texture(iVideo2x0, astuv);
        fragColor = vec4(now.r, before.g, first.b, 1.0);
    }
"""


def video_scene(source, temporal=1, fragment="video", **fields):
    """A scene class with one ShaderVideo made from `source()` (fresh keyword arguments per scene: iterators are used up)"""
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo

    class VideoScene(ShaderScene):
        def build(self):
            self.video = ShaderVideo(scene=self, **source())
            if temporal > 1:
                self.video.texture.temporal = temporal
            self.shader.fragment = fragment
    return type("VideoScene", (VideoScene,), fields)


def sources(tmp_path, clip_fps, count=40):
    """name → a callable giving ShaderVideo's keyword arguments, one per kind of source"""
    rgb, planar = rgb_clip(count), planar_clip(count)
    np.save(tmp_path/"clip.npy", rgb)
    (tmp_path/"clip.rgb").write_bytes(rgb.tobytes())
    (tmp_path/"clip.i420").write_bytes(planar.tobytes())
    with open(tmp_path/"clip.y4m", "wb") as file:
        file.write(f"YUV4MPEG2 W{CW} H{CH} F{int(clip_fps)}:1 Ip C420jpeg\n".encode())
        for frame in planar:
            file.write(b"FRAME\n" + frame.tobytes())
    return {
        "array": lambda: dict(frames=rgb, fps=clip_fps),
        "npy": lambda: dict(path=tmp_path/"clip.npy", fps=clip_fps),
        "rgb": lambda: dict(path=tmp_path/"clip.rgb", width=CW, height=CH, fps=clip_fps),
        "iterator": lambda: dict(frames=(frame for frame in rgb), width=CW, height=CH, fps=clip_fps),
        "y4m": lambda: dict(path=tmp_path/"clip.y4m"),
        "i420": lambda: dict(path=tmp_path/"clip.i420", width=CW, height=CH, fps=clip_fps),
        "planar-iterator": lambda: dict(frames=(frame for frame in planar), width=CW, height=CH, fps=clip_fps, format="i420"),
    }


def render(scene, frames, ssaa=1.0, pixel_format=None, **kwargs):
    raw = scene.main(width=W, height=H, fps=FPS, ssaa=ssaa, subsample=2, time=frames/FPS, output=bytes, pixel_format=pixel_format, **kwargs)
    per_frame = W*H*3//2 if pixel_format == "yuv420p" else W*H*3
    assert len(raw) == frames*per_frame
    return np.frombuffer(raw, np.uint8).reshape(frames, per_frame)


def assert_frames_equal(loop, sequence):
    assert loop.shape == sequence.shape
    for k in range(loop.shape[0]):
        assert np.array_equal(loop[k], sequence[k]), f"frame {k} differs"


def both_ways(Scene, frames, monkeypatch, **kwargs):
    """(frame loop scene, its frames, sequence scene, its frames)"""
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    loop = Scene()
    want = render(loop, frames, **kwargs)
    assert loop.video_sequence is None
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    scene = Scene()
    got = render(scene, frames, **kwargs)
    assert scene.video_sequence is not None and scene.video_sequence.frames == frames
    assert_frames_equal(want, got)
    return loop, want, scene, got


def assert_same_host_state(loop, scene):
    assert (scene.video._read, scene.video._exhausted) == (loop.video._read, loop.video._exhausted)
    assert (scene.time, scene.dt, scene.rdt) == (loop.time, loop.dt, loop.rdt)
    for depth in range(loop.video.texture.temporal):
        a, b = loop.video.texture.get_box(depth), scene.video.texture.get_box(depth)
        assert np.array_equal(a.texture.read(), b.texture.read()), depth
        assert a.data == b.data and a.empty == b.empty, depth


@pytest.mark.parametrize("pixel_format", ["rgb24", "yuv420p"])
@pytest.mark.parametrize("ssaa", [1.0, 2.0])
def test_video_sequence_gives_the_frame_loops_bytes(ssaa, pixel_format, monkeypatch, tmp_path):
    frames = 72                                                        # chunks of the native call: 30 frames, then what fits a quarter second
    loop, want, scene, got = both_ways(video_scene(sources(tmp_path, 30.0)["array"]), frames, monkeypatch, ssaa=ssaa, pixel_format=pixel_format)
    assert len({frame.tobytes() for frame in got}) >= frames//2 - 1     # the picture moves with the clip
    assert 34 <= scene.video._read <= 36
    assert_same_host_state(loop, scene)


@pytest.mark.parametrize("clip_fps", [20.0, 30.0, 60.0])
@pytest.mark.parametrize("kind", ["array", "npy", "rgb", "iterator", "y4m", "i420", "planar-iterator"])
def test_every_source_at_every_rate(kind, clip_fps, monkeypatch, tmp_path):
    frames = 50
    loop, want, scene, got = both_ways(video_scene(sources(tmp_path, clip_fps, count=60)[kind]), frames, monkeypatch)
    assert frames*clip_fps/FPS - 2 <= scene.video._read <= frames*clip_fps/FPS + 1 and not scene.video._exhausted
    assert (scene.video.format == "i420") == (kind in ("y4m", "i420", "planar-iterator"))
    assert len({frame.tobytes() for frame in got}) >= scene.video._read
    assert_same_host_state(loop, scene)


@pytest.mark.parametrize("kind", ["npy", "y4m"])
def test_a_temporal_matrix_through_a_translated_fragment(kind, monkeypatch, tmp_path):
    Scene = video_scene(sources(tmp_path, 30.0)[kind], temporal=3, fragment=TEMPORAL_FRAGMENT)
    loop, want, scene, got = both_ways(Scene, 48, monkeypatch)
    assert scene.shader.translated and not scene.shader.fallback
    names = {u.name for u in scene.shader.full_pipeline()}
    assert {"iVideo0x0", "iVideo1x0", "iVideo2x0"} <= names
    assert_same_host_state(loop, scene)
    # the three rows hold three different source frames: a frame drawn with another frame's bindings is another picture
    rows = [scene.video.texture.get_box(depth).texture.read() for depth in range(3)]
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])


@pytest.mark.parametrize("kind", ["array", "iterator", "y4m"])
def test_a_clip_shorter_than_the_scene_holds_its_last_frame(kind, monkeypatch, tmp_path):
    loop, want, scene, got = both_ways(video_scene(sources(tmp_path, 60.0, count=9)[kind]), 40, monkeypatch)
    assert scene.video._read == 9 and scene.video._exhausted
    assert all(np.array_equal(got[k], got[14]) for k in range(14, 40)) and not np.array_equal(got[2], got[14])
    assert_same_host_state(loop, scene)


@pytest.mark.parametrize("kind, clip_fps", [("npy", 60.0), ("i420", 30.0)])
def test_chunks_of_seven_frames(kind, clip_fps, monkeypatch, tmp_path):
    from shaderflow_amd.clockloop import ClockLoop
    monkeypatch.setattr(ClockLoop, "chunk_frames", lambda self, measured: 7)
    loop, want, scene, got = both_ways(video_scene(sources(tmp_path, clip_fps, count=60)[kind], temporal=2), 45, monkeypatch)
    assert_same_host_state(loop, scene)


def test_one_slot_filler_serves_the_frame_loop_and_the_sequence(monkeypatch):
    """`VideoStage.fill` behind `update()` and behind the sequence's reader: the same texture bytes for an rgb, an i420 and a 4:2:0
    Motion-JPEG clip of 5 frames at 40 x 24 (a partial MCU at 4:2:0; `slot_count` is at its clamp there), and the same words for a
    wrong-sized i420 frame"""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    import jpeg_ref as J
    from shaderflow_amd.videosequence import SLOTS_MAX
    w, h, count = 40, 24, 5
    rng = np.random.default_rng(7)
    rgb = rng.integers(0, 256, (count, h, w, 3), dtype=np.uint8)
    planar = rng.integers(0, 256, (count, w*h*3//2), dtype=np.uint8)
    streams = [J.encode(J.picture("noise", w, h, seed), 90) for seed in range(count)]
    clips = {"rgb": lambda: dict(frames=iter(rgb), width=w, height=h, fps=FPS),
             "i420": lambda: dict(frames=iter(planar), width=w, height=h, fps=FPS, format="i420"),
             "mjpeg": lambda: dict(frames=iter(streams), fps=FPS, format="mjpeg")}
    for kind, source in clips.items():
        loop, want, scene, got = both_ways(video_scene(source, temporal=count), count + 1, monkeypatch)      # (nothing lands on the first scene frame)
        assert scene.video._read == count and scene.video.format == (None if kind == "rgb" else kind)
        assert scene.video_sequence.video.per_chunk == SLOTS_MAX//2
        assert_same_host_state(loop, scene)                            # every box of the matrix: the five frames' texture bytes
        boxes = [scene.video.texture.get_box(depth).texture.read() for depth in range(count)]
        assert len({box.tobytes() for box in boxes}) == count, kind

    def short_frame_at_two():
        for k, frame in enumerate(planar):
            yield frame[:-1] if k == 2 else frame
    words = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", mode)
        scene = video_scene(lambda: dict(frames=short_frame_at_two(), width=w, height=h, fps=FPS, format="i420"))()
        with pytest.raises(ValueError) as raised:
            scene.main(width=W, height=H, fps=FPS, time=(count + 1)/FPS, freewheel=True)
        assert (scene.video_sequence is not None) == (mode == "1")
        words[mode] = str(raised.value)
    assert words["0"] == words["1"]
    assert all(part in words["1"] for part in ("source frame 2", f"{w} x {h}", str(w*h*3//2), str(w*h*3//2 - 1)))


def test_the_video_example_takes_the_sequence():
    from examples.scenes import Video
    scene = type("Video", (Video,), {"clip": (rgb_clip(6), 30.0)})()
    render(scene, 12)
    assert scene.video_sequence is not None and scene.video._read == 6


# ---- 3. the host objects behind a run ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["iterator", "npy", "y4m"])
def test_a_run_cut_short_leaves_the_host_objects_at_the_last_frame_drawn(kind, monkeypatch, tmp_path):
    from shaderflow_amd.clockloop import ClockLoop
    from shaderflow_amd.exporting import ExportingHelper
    made = sources(tmp_path, 60.0, count=60)
    Scene = video_scene(made[kind], temporal=2)
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    monkeypatch.setattr(ClockLoop, "chunk_frames", lambda self, measured: 7)
    looks, check, scenes = [], ExportingHelper._check_encoder, []

    def quits_on_the_third_look(self):
        looks.append(1)
        if len(looks) == 3:
            scenes[0].quit = True
        return check(self)
    scene = Scene()
    scenes.append(scene)
    monkeypatch.setattr(ExportingHelper, "_check_encoder", quits_on_the_third_look)
    scene.main(width=W, height=H, fps=FPS, time=60/FPS, freewheel=True)
    assert scene.video_sequence is not None
    # three native calls were made (the third look came in front of the third), each of one to seven frames: a call ends in front of a
    # landing the reader has not staged yet, so how long they were depends on the reader's pace
    done = scene.video_sequence.frames
    assert 3 <= done <= 21
    monkeypatch.setattr(ExportingHelper, "_check_encoder", check)
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    loop = Scene()
    loop.main(width=W, height=H, fps=FPS, time=done/FPS, freewheel=True)
    assert scene.video._read == loop.video._read and done - 3 <= scene.video._read <= done - 1
    read = scene.video._read
    assert_same_host_state(loop, scene)
    # a further update() shows the next source frame, not one the reader had taken ahead
    for one in (loop, scene):
        one.time = 1000.0
        one.video.update()
    assert scene.video._read == loop.video._read == read + 1
    shown = scene.video.texture.get_box().texture.read()
    assert np.array_equal(shown, loop.video.texture.get_box().texture.read())
    if kind != "y4m":
        assert np.array_equal(shown, np.flipud(rgb_clip(60)[read]))
    else:
        assert np.array_equal(shown, np.flipud(i420_to_rgb(planar_clip(60)[read], CW, CH)))


# ---- 4. a reader that raises -----------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
def test_a_reader_that_raises_fails_the_export_with_its_exception(monkeypatch):
    clip = rgb_clip(20)

    def decoder():
        for k, frame in enumerate(clip):
            if k == 11:
                raise OSError("the decoder went away")
            yield frame
    Scene = video_scene(lambda: dict(frames=decoder(), width=CW, height=CH, fps=60.0))
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    scene = Scene()
    with pytest.raises(OSError, match="decoder went away"):
        scene.main(width=W, height=H, fps=FPS, time=40/FPS, freewheel=True)       # (render-only: no sink is left open behind the failure)
    assert scene.video_sequence is not None
    # the frames staged before the failure were drawn: as in the frame loop, the exception comes out of the frame that wanted frame 11
    from shaderflow_amd.scheduler import freewheel_clock
    from shaderflow_amd.videosequence import landing_frames
    wanted_it = int(np.flatnonzero(landing_frames(freewheel_clock(FPS, 40, 1.0)[0], 60.0) == 11)[0])
    assert scene.video_sequence.frames == wanted_it and scene.video._read == 11 and not scene.video._exhausted
    assert np.array_equal(scene.video.texture.get_box().texture.read(), np.flipud(clip[10]))


# ---- 5. falling back -----------------------------------------------------------------------------------------------------------------

def fallback_scenes():
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    clip = rgb_clip(30)

    class Subclassed(ShaderVideo):
        pass

    class Subclass(ShaderScene):
        def build(self):
            self.video = Subclassed(scene=self, frames=clip, fps=30.0)
            self.shader.fragment = "video"

    class OwnUpdate(ShaderScene):
        def build(self):
            self.video = ShaderVideo(scene=self, frames=clip, fps=30.0)
            self.shader.fragment = "video"

        def update(self):
            pass

    class TwoVideos(ShaderScene):
        def build(self):
            self.other = ShaderVideo(scene=self, name="iOther", frames=clip[::-1], fps=20.0)
            self.video = ShaderVideo(scene=self, frames=clip, fps=30.0)
            self.shader.fragment = "video"

    class AudioBeside(ShaderScene):
        def build(self):
            from shaderflow_amd import synth
            from shaderflow_amd.audio import ShaderAudio
            self.audio = ShaderAudio(scene=self, name="iAudio")
            self.audio.load(samples=synth.sweep_clip(1.0, 44100), samplerate=44100)
            self.video = ShaderVideo(scene=self, frames=clip, fps=30.0)
            self.shader.fragment = "video"

    class TwoLayers(ShaderScene):
        def build(self):
            self.video = ShaderVideo(scene=self, frames=clip, fps=30.0)
            self.video.texture.layers = 2
            self.shader.fragment = "video"
    return {"subclass": Subclass, "own-update": OwnUpdate, "two-videos": TwoVideos, "audio-beside": AudioBeside, "two-layers": TwoLayers}


@pytest.mark.parametrize("case", ["subclass", "own-update", "two-videos", "audio-beside", "two-layers"])
def test_scenes_the_sequence_does_not_take_keep_the_frame_loop(case, monkeypatch):
    Scene = fallback_scenes()[case]
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    want = render(Scene(), 30, batch=False)
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    scene = Scene()
    from shaderflow_amd.sequence import Sequence
    got = render(scene, 30)
    assert scene.video_sequence is None
    scene.freewheel = True
    if case == "audio-beside":
        assert Sequence.taken(scene) != "video_sequence"                # (a video beside audio may be the join's)
    else:
        assert not Sequence.applicable(scene)
    assert_frames_equal(want, got)
    assert scene.video._read >= 13 and scene.video.texture.get_box().texture.read().any()      # the host module wrote its texture
