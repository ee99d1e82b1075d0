"""
Motion-JPEG sources on the device (csrc/jpeg_decode_kernels.hpp, csrc/capi_video_jpeg.hip, shaderflow_amd/mjpegsource.py):

  1. the kernels through sfx_jpeg_decode on every stored stream: the coefficients are tests/jpeg_ref.py's exactly; the planes are the
     float64 restatement's wherever the value in front of the rounding is more than 1e-3 from a tie, within 1 elsewhere; the RGB bytes
     are the restatement's upsampling and colour applied to the device's OWN planes, byte for byte.
     The band: a sample is a sum of 64 products of a coefficient (|c q| ≤ 2^11·255 is the format's bound, the stored streams stay below
     2^11) and two basis factors ≤ 1/2, added in f32 (2^-24 relative per operation, 16 operations deep): the error is below
     16 · 2^-24 · Σ|terms| ≤ 16 · 2^-24 · 2^11 · 8 ≈ 1.6e-2 in the worst case the format allows, and about 2^-24 · 16 · 300 ≈ 3e-4 at
     the magnitudes of these 8-bit pictures (Σ|terms| of a block stays near its samples' range), inside the 1e-3 the issue sets;
  2. a decoded frame lands bottom-up in the texture and a temporal matrix rolls; damaged scans set the status, raise RuntimeError from
     update() and from an export, and the frame behind them decodes;
  3. a scene with an `.avi` source: the frame loop and the video sequence, alone and joined (beside audio), give the same bytes; a clip
     shorter than the scene holds its last frame; an exported `.avi` read back shows the device decode of that file's frames.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_decode_ref as D  # noqa: E402
import jpeg_ref as J  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent/"golden"/"jpeg_streams.npz"
FPS = 60.0
W, H = 96, 54
CW, CH = 48, 32


def stored() -> dict:
    data = np.load(GOLDEN)
    return {name[:-7]: data[name].tobytes() for name in data.files if name.endswith(".stream")}


STREAMS = stored()
_reference: dict = {}


def reference(name: str) -> dict:
    """The restatement of a stored stream, computed once"""
    if name not in _reference:
        _reference[name] = D.decode(STREAMS[name])
    return _reference[name]


# ---- 1. the kernels --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(STREAMS))
def test_the_kernels_against_the_restatement(name):
    from shaderflow_amd.mjpegsource import device_decode
    want = reference(name)
    got = device_decode(STREAMS[name])
    header = got["header"]
    assert got["status"] == 0
    coefficients = want["coefficients"].reshape(-1, *want["coefficients"].shape[2:])
    assert np.array_equal(got["coefficients"], coefficients)
    planes = D.split_planes(got["planes"], header.width, header.height, header.components, header.sampling)
    near = 0
    for mine, theirs, samples in zip(planes, want["planes"], want["samples"]):
        tie = np.abs(samples - np.floor(samples) - 0.5) < 1e-3
        near += int(tie.sum())
        difference = np.abs(mine.astype(np.int32) - theirs.astype(np.int32))
        print(f"{name}: {int(tie.sum())} samples near a tie, {int((difference > 0).sum())} differ, max {difference.max()}")
        assert not difference[~tie].any() and difference.max() <= 1
    assert near <= 0.01*sum(plane.size for plane in planes)
    assert np.array_equal(got["rgb"], D.to_rgb(planes, header.width, header.height, header.sampling))


def damaged() -> dict:
    """name → a stream whose scan is bad in one way, and the status bits the bounded reader may set: exactly these when `exact`, else
    at least one of them and no other (what garbage decodes as depends on the bytes that are left)"""
    from shaderflow_amd.mjpegsource import parse_header
    base = STREAMS["wide_420"]                                         # restart interval 3 MCUs, the standard's tables
    start = parse_header(base).scan_start
    first = base.index(b"\xff\xd0", start)
    truncated = base[:start + (len(base) - start)//2]                  # no EOI, the later intervals' markers are gone
    # an unassigned code: the standard's DC luminance table leaves the 9-bit prefix of all ones unassigned
    unassigned = base[:start] + b"\xff\x00\xff\x00" + base[start + 4:]
    wrong = base[:first + 1] + b"\xd3" + base[first + 2:]
    short = base[:first - 6] + base[first:]                            # the first interval loses its last bytes
    # unassigned: the first lane stops at its first symbol, every other interval is whole. wrong-rst: only the interval behind the
    # marker is refused, before it reads a bit
    return {"truncated": (truncated, 4 | 8, False), "unassigned": (unassigned, 1, True), "wrong-rst": (wrong, 4, True), "short-interval": (short, 1 | 2 | 8, False)}


@pytest.mark.parametrize("case", ["truncated", "unassigned", "wrong-rst", "short-interval"])
def test_a_damaged_scan_sets_the_status_and_nothing_else(case):
    from shaderflow_amd.mjpegsource import device_decode
    stream, bits, exact = damaged()[case]
    got = device_decode(stream)
    print(f"{case}: status {got['status']}")
    assert got["status"] == bits if exact else (got["status"] & bits and not got["status"] & ~bits)
    assert not got["rgb"].any()                                        # a frame with a bad status is not drawn
    assert device_decode(STREAMS["wide_420"])["status"] == 0            # the context goes on


# ---- 2. the stage ----------------------------------------------------------------------------------------------------------------------

class Stage:
    """sfx_video_* with SFX_VIDEO_MJPEG over `temporal` bare RGB8 textures of the default context"""

    def __init__(self, header, capacity, temporal=1, slots=2):
        from shaderflow_amd import _native as N
        self.N, self.lib, self.header = N, N.lib(), header
        self.context = N.default_context()
        self.textures = []
        for _ in range(temporal):
            handle = N.Handle()
            N.check(self.lib.sfx_texture_create(self.context.handle, header.width, header.height, 3, N.U8, C.byref(handle)))
            self.textures.append(handle)
        self.handle = N.Handle()
        boxes = (N.Handle*temporal)(*self.textures)
        N.check(self.lib.sfx_video_create_mjpeg(self.context.handle, boxes, temporal, header.width, header.height, header.components,
                                                header.sampling[0], header.sampling[1], capacity, slots, C.byref(self.handle)))

    def view(self, slot):
        pointer, nbytes = C.c_void_p(), C.c_size_t()
        self.N.check(self.lib.sfx_video_slot(self.handle, slot, C.byref(pointer), C.byref(nbytes)))
        return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint8)), shape=(nbytes.value,))

    def show(self, stream, slot=0):
        from shaderflow_amd.mjpegsource import stage
        self.N.check(self.lib.sfx_video_submit_bytes(self.handle, slot, stage(stream, self.header, self.view(slot))))
        self.N.check(self.lib.sfx_video_step(self.handle, slot))

    def bad(self, wait=True):
        frame, status = C.c_int64(), C.c_uint32()
        self.N.check(self.lib.sfx_video_status(self.handle, 1 if wait else 0, C.byref(frame), C.byref(status)))
        return frame.value, status.value

    def read(self, index=0):
        out = np.empty((self.header.height, self.header.width, 3), np.uint8)
        self.N.check(self.lib.sfx_texture_read(self.textures[index], out.ctypes.data, out.nbytes))
        return out

    def close(self):
        self.lib.sfx_video_destroy(self.handle)
        for texture in self.textures:
            self.lib.sfx_texture_destroy(texture)


@pytest.mark.parametrize("name", ["partial_420", "odd_422", "wide_420", "mid_444", "long_grey", "tall_420"])
def test_a_frame_lands_bottom_up_in_the_texture(name):
    from shaderflow_amd.mjpegsource import capacity_for, device_decode, parse_header
    header = parse_header(STREAMS[name])
    stage = Stage(header, capacity_for(header, len(STREAMS[name])))
    try:
        stage.show(STREAMS[name])
        assert stage.bad() == (-1, 0)
        assert np.array_equal(stage.read(), np.flipud(device_decode(STREAMS[name])["rgb"]))
    finally:
        stage.close()


def test_a_temporal_matrix_rolls_and_a_damaged_frame_is_passed_over():
    from shaderflow_amd import _native as N
    from shaderflow_amd.mjpegsource import capacity_for, device_decode, parse_header
    frames = [J.encode(J.picture("noise", CW, CH, seed), 90) for seed in range(5)]
    pictures = [np.flipud(device_decode(frame)["rgb"]) for frame in frames]
    header = parse_header(frames[0])
    stage = Stage(header, capacity_for(header, None), temporal=3, slots=2)
    try:
        for k, frame in enumerate(frames):
            stage.show(frame, slot=k % 2)
        # create order [0, 1, 2]: frame k is written into the box that was oldest: 2, 1, 0, 2, 1
        assert np.array_equal(stage.read(1), pictures[4]) and np.array_equal(stage.read(2), pictures[3]) and np.array_equal(stage.read(0), pictures[2])
        assert stage.bad() == (-1, 0)
        bad, bits, _ = damaged()["truncated"]                             # (same geometry as the clip)
        stage.show(bad, slot=1)                                        # lands as frame 5, into box 0: which keeps frame 2
        stage.show(frames[0], slot=0)                                  # frame 6, into box 2
        frame, status = stage.bad()
        assert frame == 5 and status & bits
        assert stage.bad() == (-1, 0)                                  # asked once
        assert np.array_equal(stage.read(0), pictures[2]) and np.array_equal(stage.read(2), pictures[0])
        # the protocol's refusals by return code
        lib = stage.lib
        assert lib.sfx_video_submit(stage.handle, 0) != N.OK           # a compressed frame needs its length
        view = stage.view(0)
        view[:4] = 0
        assert lib.sfx_video_submit_bytes(stage.handle, 0, 4096) != N.OK and b"magic" in lib.sfx_last_error()
        assert lib.sfx_video_submit_bytes(stage.handle, 0, view.size + 16) != N.OK
        handle = N.Handle()
        boxes = (N.Handle*1)(stage.textures[0])
        assert lib.sfx_video_create_mjpeg(stage.context.handle, boxes, 1, CW, CH, 3, 1, 2, 1 << 16, 1, C.byref(handle)) != N.OK      # 1x2 sampling
        assert lib.sfx_video_create_mjpeg(stage.context.handle, boxes, 1, CW, CH, 4, 1, 1, 1 << 16, 1, C.byref(handle)) != N.OK      # CMYK
        assert lib.sfx_video_create(stage.context.handle, boxes, 1, CW, CH, N.VIDEO_MJPEG, 1, C.byref(handle)) != N.OK               # not this call's
    finally:
        stage.close()


# ---- 3. scenes -------------------------------------------------------------------------------------------------------------------------

def clip_frames(count, seed=0):
    return [J.encode(J.picture("noise", CW, CH, seed + k), 90) for k in range(count)]


def write_avi(path, frames, fps):
    from shaderflow_amd.mjpeg import AviWriter
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        writer = AviWriter(fd, CW, CH, fps)
        writer.begin()
        for frame in frames:
            writer.add(frame)
        writer.finish()
    finally:
        os.close(fd)


def video_scene(source, audio=False, temporal=1):
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo

    class VideoScene(ShaderScene):
        def build(self):
            if audio:
                from shaderflow_amd import synth
                from shaderflow_amd.audio import ShaderAudio
                self.audio = ShaderAudio(scene=self, name="iAudio")
                self.audio.load(samples=synth.sweep_clip(1.0, 44100), samplerate=44100)
            self.video = ShaderVideo(scene=self, **source())
            if temporal > 1:
                self.video.texture.temporal = temporal
            self.shader.fragment = "video"
    return VideoScene


def render(scene, frames):
    raw = scene.main(width=W, height=H, fps=FPS, subsample=2, time=frames/FPS, output=bytes)
    assert len(raw) == frames*W*H*3
    return np.frombuffer(raw, np.uint8).reshape(frames, -1)


@pytest.mark.parametrize("kind", ["avi", "mjpeg", "bytes"])
def test_the_three_loops_give_the_same_bytes(kind, monkeypatch, tmp_path):
    frames, count = 40, 30
    clip = clip_frames(count)
    write_avi(tmp_path/"clip.avi", clip, 30.0)
    (tmp_path/"clip.mjpeg").write_bytes(b"".join(clip))
    source = {"avi": lambda: dict(path=tmp_path/"clip.avi"), "mjpeg": lambda: dict(path=tmp_path/"clip.mjpeg", fps=30.0),
              "bytes": lambda: dict(frames=iter(clip), fps=30.0, format="mjpeg")}[kind]
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    loop = video_scene(source)()
    want = render(loop, frames)
    assert loop.video_sequence is None and loop.video.format == "mjpeg" and loop.video.fps == 30.0
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    scene = video_scene(source)()
    got = render(scene, frames)
    assert scene.video_sequence is not None and scene.video_sequence.frames == frames
    assert np.array_equal(want, got)
    assert scene.video._read == loop.video._read and 18 <= scene.video._read <= 21 and len({frame.tobytes() for frame in got}) >= scene.video._read
    assert np.array_equal(scene.video.texture.get_box().texture.read(), loop.video.texture.get_box().texture.read())
    # a further update() shows the next source frame, not one the reader took ahead: they went back as bytes
    from shaderflow_amd.mjpegsource import device_decode
    read = scene.video._read
    scene.time = 1000.0
    scene.video.update()
    assert np.array_equal(scene.video.texture.get_box().texture.read(), np.flipud(device_decode(clip[read])["rgb"]))
    if kind != "avi":
        return
    joined_loop, joined = video_scene(source, audio=True)(), video_scene(source, audio=True)()
    monkeypatch.setenv("SHADERFLOW_VIDEO_JOIN", "0")
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    beside_audio = render(joined_loop, frames)
    monkeypatch.setenv("SHADERFLOW_VIDEO_JOIN", "1")
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    got = render(joined, frames)
    assert joined.video_join is not None and joined_loop.video_join is None
    assert np.array_equal(beside_audio, got) and len({frame.tobytes() for frame in got}) >= joined.video._read


def test_a_clip_shorter_than_the_scene_holds_its_last_frame(monkeypatch, tmp_path):
    write_avi(tmp_path/"clip.avi", clip_frames(9), 60.0)
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    scene = video_scene(lambda: dict(path=tmp_path/"clip.avi"), temporal=2)()
    got = render(scene, 40)
    assert scene.video_sequence is not None and scene.video._read == 9 and scene.video._exhausted
    assert all(np.array_equal(got[k], got[14]) for k in range(14, 40)) and not np.array_equal(got[2], got[14])
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    assert np.array_equal(render(video_scene(lambda: dict(path=tmp_path/"clip.avi"), temporal=2)(), 40), got)


def test_an_exported_avi_reads_back(monkeypatch, tmp_path):
    from shaderflow_amd.mjpegsource import AviReader, device_decode
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    first = video_scene(lambda: dict(frames=np.random.default_rng(3).integers(0, 256, (12, CH, CW, 3), dtype=np.uint8), fps=60.0))()
    first.main(width=W, height=H, fps=FPS, subsample=2, time=12/FPS, output=str(tmp_path/"out.avi"), pixel_format="mjpeg")
    reader = AviReader(tmp_path/"out.avi")
    frames = list(reader)
    assert (reader.width, reader.height, reader.fps, len(frames)) == (W, H, FPS, 12)

    class Back(ShaderScene):
        def build(self):
            self.video = ShaderVideo(scene=self, path=tmp_path/"out.avi")
            self.shader.fragment = "video"
    scene = Back()
    render(scene, 8)
    assert scene.video_sequence is not None and (scene.video.width, scene.video.height) == (W, H)
    read = scene.video._read
    assert 6 <= read <= 8
    assert np.array_equal(scene.video.texture.get_box().texture.read(), np.flipud(device_decode(frames[read - 1])["rgb"]))


@pytest.mark.parametrize("case", ["truncated", "unassigned"])
def test_a_damaged_frame_raises_and_the_next_one_decodes(case, monkeypatch):
    from shaderflow_amd.mjpegsource import device_decode
    good = STREAMS["wide_420"]
    bad = damaged()[case][0]
    clip = [good, good, bad] + [good]*20
    # the frame loop: update() raises for the frame, and shows the next one
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    scene = video_scene(lambda: dict(frames=iter(clip), fps=60.0, format="mjpeg"))()
    with pytest.raises(RuntimeError, match="source frame 2 could not be decoded"):
        scene.main(width=W, height=H, fps=FPS, time=10/FPS, freewheel=True)       # (render-only: no sink is left open behind the failure)
    scene.time = 1000.0
    scene.video.update()
    assert scene.video._read == 4 and np.array_equal(scene.video.texture.get_box().texture.read(), np.flipud(device_decode(good)["rgb"]))
    # the sequence: the export fails with the same words, and the context goes on
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    scene = video_scene(lambda: dict(frames=iter(clip), fps=60.0, format="mjpeg"))()
    with pytest.raises(RuntimeError, match="source frame 2 could not be decoded"):
        scene.main(width=W, height=H, fps=FPS, time=20/FPS, freewheel=True)
    assert scene.video_sequence is not None
    assert device_decode(good)["status"] == 0
    again = video_scene(lambda: dict(frames=iter([good]*12), fps=60.0, format="mjpeg"))()
    assert render(again, 10).any()
