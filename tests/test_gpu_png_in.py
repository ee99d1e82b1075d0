"""
PNG sources on the device (csrc/png_decode_kernels.hpp, csrc/capi_video_png.hip, shaderflow_amd/pngsource.py):

  1. the kernels through sfx_png_decode on every case of tests/png_decode_ref.py's table, on the serial path and, where the case
     allows, the segment path: the inflated stream is zlib.decompress's byte for byte, the pixels are Pillow's;
  2. which path decoded a frame: the segment path this project's own stream and Z_FULL_FLUSH cuts; the serial path, fallen back to,
     a Z_SYNC_FLUSH cut with a back reference across it, Pillow's mid-block cuts at level 0, and a cut behind 00 00 FF FF inside a
     stored block — the pictures are equal all the same;
  3. damage, a case per status bit: the bit is set, the pixels stay as they were, and the 64 guard bytes sfx_png_decode keeps behind
     the inflated stream and behind the pixels on the device are untouched (it returns SFX_E_HIP otherwise), as are guards round the
     host buffers;
  4. in the texture: a frame lands bottom-up, a temporal matrix rolls, a damaged frame is passed over, the three loops give the same
     bytes from `clip.avi` and from `bytes`, a short clip holds its last frame;
  5. the round trip: a scene exported with pixel_format="png" and its sound track, played back through a second scene, is the first
     scene's frames exactly, every frame on the segment path;
  6. a PNG handle beside a Motion-JPEG handle: each decoder counts, reports and frees what is its own.
"""
from __future__ import annotations

import ctypes as C
import io
import os
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import png_decode_ref as D  # noqa: E402
import png_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = D.cases()
FPS = 60.0
W, H = 96, 54
CW, CH = 48, 32
_wanted: dict = {}


def wanted(name: str):
    """(zlib's inflated stream, Pillow's pixels) of a case, computed once"""
    if name not in _wanted:
        from PIL import Image
        stream = CASES[name]["stream"]
        width, height = D.split(stream)[:2]
        inflated = zlib.decompress(b"".join(data for kind, data, _ in P.chunks(stream)[0] if kind == b"IDAT"))
        _wanted[name] = (np.frombuffer(inflated, np.uint8).reshape(height, 1 + 3*width), np.asarray(Image.open(io.BytesIO(stream)).convert("RGB")))
    return _wanted[name]


# ---- 1. the kernels --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_the_kernels_against_zlib_and_pillow(name):
    from shaderflow_amd.pngsource import device_decode
    filtered, rgb = wanted(name)
    for segments in CASES[name]["paths"]:
        got = device_decode(CASES[name]["stream"], segments=segments)
        print(f"{name}: segments={segments}: status {got['status']}, {got['info']}")
        assert got["status"] == 0
        assert np.array_equal(got["filtered"], filtered)
        assert np.array_equal(got["rgb"], rgb)
        assert got["info"]["parallel"] + got["info"]["fell_back"] == (1 if segments else 0)


# ---- 2. paths --------------------------------------------------------------------------------------------------------------------------

def test_which_path_decodes_a_frame(monkeypatch):
    from shaderflow_amd.pngsource import device_decode
    monkeypatch.delenv("SHADERFLOW_PNG_SEGMENTS", raising=False)
    for name in D.PARALLEL:
        got = device_decode(CASES[name]["stream"])
        assert got["info"]["parallel"] == 1 and got["info"]["fell_back"] == 0 and got["info"]["segments"] == D.decode(CASES[name]["stream"])["info"]["segments"], name
        assert np.array_equal(got["rgb"], wanted(name)[1])
    for name in D.FELL_BACK:
        got = device_decode(CASES[name]["stream"], segments=True)
        assert got["info"]["parallel"] == 0 and got["info"]["fell_back"] == 1 and got["status"] == 0, name
        assert np.array_equal(got["rgb"], wanted(name)[1]) and np.array_equal(got["filtered"], wanted(name)[0])
        assert device_decode(CASES[name]["stream"])["info"] == D.decode(CASES[name]["stream"])["info"], name       # what a handle would choose
    # a one-segment stream on the segment path; and the switch
    got = device_decode(CASES["pillow-9"]["stream"], segments=True)
    assert got["info"] == {"segments": 1, "parallel": 1, "fell_back": 0} and np.array_equal(got["rgb"], wanted("pillow-9")[1])
    monkeypatch.setenv("SHADERFLOW_PNG_SEGMENTS", "0")
    assert device_decode(CASES["own-86x129"]["stream"])["info"]["parallel"] == 0
    monkeypatch.setenv("SHADERFLOW_PNG_SEGMENTS", "1")
    assert device_decode(CASES["zlib-86x129"]["stream"])["info"]["parallel"] == 1


# ---- 3. damage -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(D.damaged()))
def test_damage_sets_its_bit_and_nothing_else_is_written(name):
    from shaderflow_amd import _native as N
    from shaderflow_amd import pngsource as S
    stream, bit = D.damaged()[name]
    header = S.parse_header(stream)
    view = np.zeros(S.capacity_for(header, len(stream)), np.uint8)
    total = S.stage(stream, header, view)
    filtered_bytes, rgb_bytes = header.filtered_bytes, header.width*header.height*3
    filtered, rgb = np.full(filtered_bytes + 128, 0x5a, np.uint8), np.full(rgb_bytes + 128, 0x5a, np.uint8)
    for mode in (0, 1):
        status, words = C.c_uint32(0), (C.c_uint32*3)()
        rgb[64:64 + rgb_bytes] = 0x11
        N.check(N.lib().sfx_png_decode(N.default_context().handle, view.ctypes.data, total, header.width, header.height, mode,
                                       filtered[64:].ctypes.data, rgb[64:].ctypes.data, C.byref(status), words))     # (SFX_E_HIP: a device guard byte was written)
        print(f"{name}: mode {mode}: status {status.value}, info {list(words)}")
        assert status.value == bit == D.decode(stream, segments=bool(mode))["status"]
        assert not rgb[64:64 + rgb_bytes].any()                        # a frame with a bad status is not drawn
        assert (filtered[:64] == 0x5a).all() and (filtered[64 + filtered_bytes:] == 0x5a).all() and (rgb[:64] == 0x5a).all() and (rgb[64 + rgb_bytes:] == 0x5a).all()
        want = D.decode(stream, segments=bool(mode))["info"]           # (damaged deflate data never validates: the serial path says what is wrong)
        assert list(words) == [want["segments"], want["parallel"], want["fell_back"]]
    assert S.device_decode(CASES["own-37x21"]["stream"])["status"] == 0  # the context goes on


def test_a_staged_frame_is_validated_before_the_kernels_see_it():
    """SFX_PNG_BAD_DESCRIPTOR is the kernels' own second look; the C-ABI refuses such a frame first, naming what is wrong"""
    from shaderflow_amd import _native as N
    from shaderflow_amd import pngsource as S
    stream = CASES["own-37x21"]["stream"]
    header = S.parse_header(stream)
    view = np.zeros(S.capacity_for(header, len(stream)), np.uint8)
    total = S.stage(stream, header, view)
    lib, status = N.lib(), C.c_uint32(0)

    def refused(changed, words, width=37):
        code = lib.sfx_png_decode(N.default_context().handle, changed.ctypes.data, total, width, 21, -1, None, None, C.byref(status), None)
        assert code != N.OK and words in lib.sfx_last_error(), lib.sfx_last_error()
    for field, value, words in (("magic", 0x444a4653, b"magic"), ("segments", 0, b"segment table"), ("segments", 1000, b"segment table"),
                                ("payload_offset", 40, b"segment table"), ("payload_bytes", total, b"payload"), ("height", 22, b"width or height")):
        changed = view.copy()
        changed[:S.FRAME_FIXED].view(S.STAGED)[0][field] = value
        refused(changed, words)
    changed = view.copy()
    changed[S.FRAME_FIXED + 4:S.FRAME_FIXED + 8].view("<u4")[0] = total     # the second segment starts behind the payload
    refused(changed, b"ascend")
    changed = view.copy()
    changed[S.FRAME_FIXED + 8:S.FRAME_FIXED + 12].view("<u4")[0] = 1        # … the third in front of the second
    refused(changed, b"ascend")
    refused(view, b"width or height", width=36)


# ---- 4. in the texture -----------------------------------------------------------------------------------------------------------------

class Stage:
    """sfx_video_* with SFX_VIDEO_PNG (`codec`: another source module's format) over `temporal` bare RGB8 textures of the default context"""

    def __init__(self, header, capacity, temporal=1, slots=2, codec=None):
        from shaderflow_amd import _native as N
        from shaderflow_amd import pngsource
        self.N, self.lib, self.header, self.codec = N, N.lib(), header, codec or pngsource
        self.context = N.default_context()
        self.textures = []
        for _ in range(temporal):
            handle = N.Handle()
            N.check(self.lib.sfx_texture_create(self.context.handle, header.width, header.height, 3, N.U8, C.byref(handle)))
            self.textures.append(handle)
        self.handle = self.codec.create(self.context.handle, (N.Handle*temporal)(*self.textures), temporal, header, capacity, slots)

    def view(self, slot):
        pointer, nbytes = C.c_void_p(), C.c_size_t()
        self.N.check(self.lib.sfx_video_slot(self.handle, slot, C.byref(pointer), C.byref(nbytes)))
        return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint8)), shape=(nbytes.value,))

    def show(self, stream, slot=0):
        self.N.check(self.lib.sfx_video_submit_bytes(self.handle, slot, self.codec.stage(stream, self.header, self.view(slot))))
        self.N.check(self.lib.sfx_video_step(self.handle, slot))

    def bad(self, wait=True):
        frame, status = C.c_int64(), C.c_uint32()
        self.N.check(self.lib.sfx_video_status(self.handle, 1 if wait else 0, C.byref(frame), C.byref(status)))
        return frame.value, status.value

    def paths(self, entry="sfx_video_png_paths"):
        parallel, serial = C.c_uint64(7), C.c_uint64(7)
        self.N.check(getattr(self.lib, entry)(self.handle, C.byref(parallel), C.byref(serial)))
        return parallel.value, serial.value

    def read(self, index=0):
        out = np.empty((self.header.height, self.header.width, 3), np.uint8)
        self.N.check(self.lib.sfx_texture_read(self.textures[index], out.ctypes.data, out.nbytes))
        return out

    def close(self):
        self.lib.sfx_video_destroy(self.handle)
        for texture in self.textures:
            self.lib.sfx_texture_destroy(texture)


@pytest.mark.parametrize("name", ["own-86x129", "own-8x1100", "zlib-3000x3", "pillow-9", "own-1x7", "filter-4", "sync-flush"])
def test_a_frame_lands_bottom_up_in_the_texture(name):
    from shaderflow_amd.pngsource import capacity_for, parse_header
    stream = CASES[name]["stream"]
    header = parse_header(stream)
    stage = Stage(header, capacity_for(header, len(stream)))
    try:
        stage.show(stream)
        assert stage.bad() == (-1, 0)
        assert np.array_equal(stage.read(), np.flipud(wanted(name)[1]))
        want = D.decode(stream)["info"]
        assert stage.paths() == (want["parallel"], 1 - want["parallel"])
    finally:
        stage.close()


def clip_pictures(count, seed=0, width=CW, height=CH):
    return [D.mixed(width, height, seed + k) for k in range(count)]


def test_a_temporal_matrix_rolls_and_a_damaged_frame_is_passed_over():
    from shaderflow_amd import _native as N
    from shaderflow_amd.pngsource import BAD_ADLER, capacity_for, parse_header
    pictures = clip_pictures(5)
    frames = [P.encode(picture) for picture in pictures]
    flipped = [np.flipud(picture) for picture in pictures]
    header = parse_header(frames[0])
    stage = Stage(header, capacity_for(header, None), temporal=3, slots=2)
    try:
        for k, frame in enumerate(frames):
            stage.show(frame, slot=k % 2)
        # create order [0, 1, 2]: frame k is written into the box that was oldest: 2, 1, 0, 2, 1
        assert np.array_equal(stage.read(1), flipped[4]) and np.array_equal(stage.read(2), flipped[3]) and np.array_equal(stage.read(0), flipped[2])
        assert stage.bad() == (-1, 0)
        bad = frames[1][:-17] + bytes([frames[1][-17] ^ 1]) + frames[1][-16:]      # the Adler-32's last byte: in front of the last IDAT's CRC and IEND's 12 bytes
        stage.show(bad, slot=1)                                        # lands as frame 5, into box 0: which keeps frame 2
        stage.show(frames[0], slot=0)                                  # frame 6, into box 2
        assert stage.bad() == (5, BAD_ADLER)
        assert stage.bad() == (-1, 0)                                  # asked once
        assert np.array_equal(stage.read(0), flipped[2]) and np.array_equal(stage.read(2), flipped[0])
        assert stage.paths() == (7, 0)
        # the protocol's refusals by return code
        lib = stage.lib
        assert lib.sfx_video_submit(stage.handle, 0) != N.OK           # a compressed frame needs its length
        view = stage.view(0)
        view[:4] = 0
        assert lib.sfx_video_submit_bytes(stage.handle, 0, 4096) != N.OK and b"magic" in lib.sfx_last_error()
        assert lib.sfx_video_submit_bytes(stage.handle, 0, view.size + 16) != N.OK
        handle = N.Handle()
        boxes = (N.Handle*1)(stage.textures[0])
        assert lib.sfx_video_create(stage.context.handle, boxes, 1, CW, CH, N.VIDEO_PNG, 1, C.byref(handle)) != N.OK                   # not this call's
        assert lib.sfx_video_create_png(stage.context.handle, boxes, 1, CW, CH, 16, 1, C.byref(handle)) != N.OK                        # no room for a record
        assert lib.sfx_video_create_png(stage.context.handle, boxes, 1, CW + 1, CH, 1 << 16, 1, C.byref(handle)) != N.OK               # not the texture's size
    finally:
        stage.close()


def write_avi(path, frames, fps, width=CW, height=CH):
    from shaderflow_amd.mjpeg import AviWriter
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        writer = AviWriter(fd, width, height, fps, fourcc=b"MPNG")
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


def render(scene, frames, width=W, height=H, subsample=2):
    raw = scene.main(width=width, height=height, fps=FPS, subsample=subsample, time=frames/FPS, output=bytes)
    assert len(raw) == frames*width*height*3
    return np.frombuffer(raw, np.uint8).reshape(frames, -1)


@pytest.mark.parametrize("kind", ["avi", "bytes"])
def test_the_three_loops_give_the_same_bytes(kind, monkeypatch, tmp_path):
    frames, count = 40, 30
    pictures = clip_pictures(count)
    clip = [P.encode(picture) if k % 3 else D.deflated(D.filtered_of(picture)) for k, picture in enumerate(pictures)]      # both paths in one clip
    write_avi(tmp_path/"clip.avi", clip, 30.0)
    source = {"avi": lambda: dict(path=tmp_path/"clip.avi"), "bytes": lambda: dict(frames=iter(clip), fps=30.0, format="png")}[kind]
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    loop = video_scene(source)()
    want = render(loop, frames)
    assert loop.video_sequence is None and loop.video.format == "png" and loop.video.fps == 30.0
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    scene = video_scene(source)()
    got = render(scene, frames)
    assert scene.video_sequence is not None and scene.video_sequence.frames == frames
    assert np.array_equal(want, got)
    assert scene.video._read == loop.video._read and 18 <= scene.video._read <= 21 and len({frame.tobytes() for frame in got}) >= scene.video._read
    assert np.array_equal(scene.video.texture.get_box().texture.read(), np.flipud(pictures[scene.video._read - 1]))
    # a further update() shows the next source frame, not one the reader took ahead: they went back as bytes
    read = scene.video._read
    scene.time = 1000.0
    scene.video.update()
    assert np.array_equal(scene.video.texture.get_box().texture.read(), np.flipud(pictures[read]))
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
    write_avi(tmp_path/"clip.avi", [P.encode(picture) for picture in clip_pictures(9)], 60.0)
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    scene = video_scene(lambda: dict(path=tmp_path/"clip.avi"), temporal=2)()
    got = render(scene, 40)
    assert scene.video_sequence is not None and scene.video._read == 9 and scene.video._exhausted
    assert all(np.array_equal(got[k], got[14]) for k in range(14, 40)) and not np.array_equal(got[2], got[14])
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    assert np.array_equal(render(video_scene(lambda: dict(path=tmp_path/"clip.avi"), temporal=2)(), 40), got)


def test_a_damaged_frame_raises_and_the_next_one_decodes(monkeypatch):
    pictures = clip_pictures(2)
    good, other = P.encode(pictures[0]), P.encode(pictures[1])
    whole = D.deflated(D.filtered_of(pictures[0]))
    bad = whole[:len(whole)//2] + whole[-16:]                          # IDAT cut short inside (the chunk length no longer fits: the parser…)
    bad = D.png(CW, CH, [zlib.compress(D.filtered_of(pictures[0]).tobytes())[:-40] + bytes(4)])      # … so: a stream that runs out of bits
    clip = [good, good, bad, other] + [good]*20
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    scene = video_scene(lambda: dict(frames=iter(clip), fps=60.0, format="png"))()
    with pytest.raises(RuntimeError, match="source frame 2 could not be decoded: .*ran out of bits"):
        scene.main(width=W, height=H, fps=FPS, time=10/FPS, freewheel=True)       # (render-only: no sink is left open behind the failure)
    scene.time = 1000.0
    scene.video.update()
    assert scene.video._read == 4 and np.array_equal(scene.video.texture.get_box().texture.read(), np.flipud(pictures[1]))
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    scene = video_scene(lambda: dict(frames=iter(clip), fps=60.0, format="png"))()
    with pytest.raises(RuntimeError, match="source frame 2 could not be decoded"):
        scene.main(width=W, height=H, fps=FPS, time=20/FPS, freewheel=True)
    assert scene.video_sequence is not None
    again = video_scene(lambda: dict(frames=iter([good]*12), fps=60.0, format="png"))()
    assert render(again, 10).any()


# ---- 5. the round trip -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width, height", [(64, 36), (160, 90)])
def test_an_exported_clip_played_back_is_the_first_scene(width, height, monkeypatch, tmp_path):
    from shaderflow_amd.audio import ShaderAudio
    from shaderflow_amd.pngsource import AviReader
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    monkeypatch.delenv("SHADERFLOW_PNG_SEGMENTS", raising=False)
    count = 12
    source = np.random.default_rng(3).integers(0, 256, (count, height, width, 3), dtype=np.uint8)
    source[:, : height//2] = (np.arange(width)[None, None, :, None]*np.array([1, 2, 3]) + np.arange(count)[:, None, None, None]).astype(np.uint8)   # smooth above, noise below
    make = video_scene(lambda: dict(frames=source, fps=FPS), audio=True)
    # (raw frames leave a scene bottom row first, as the reference pipes them to ffmpeg; a PNG file holds the top row first)
    want = np.frombuffer(make().main(width=width, height=height, fps=FPS, time=count/FPS, output=bytes), np.uint8).reshape(count, height, width, 3)[:, ::-1]
    make().main(width=width, height=height, fps=FPS, time=count/FPS, output=str(tmp_path/"out.avi"), pixel_format="png", sound_track=True)
    reader = AviReader(tmp_path/"out.avi")
    assert (reader.width, reader.height, reader.fps, len(reader)) == (width, height, FPS, count)
    reader.close()

    class Back(ShaderScene):
        def build(self):
            self.audio = ShaderAudio(scene=self, name="iAudio")
            self.audio.file = tmp_path/"out.avi"                       # the same file's PCM track
            self.video = ShaderVideo(scene=self, path=tmp_path/"out.avi")
            self.shader.fragment = "video"
    # the file's frames, one by one, as the video plays them into its texture: decode(encode(frame)) is the frame. (What the scene
    # draws from that texture is the fragment's resampling of it, which is not the identity, so the comparison stands at the texture.)
    scene = Back()
    scene.main(width=width, height=height, fps=FPS, time=1/FPS, output=bytes)        # (its one frame is drawn at time 0: nothing is read yet)
    assert scene.video.format == "png" and (scene.video.width, scene.video.height, scene.video.fps) == (width, height, FPS)
    assert scene.video._read == 0
    for k in range(count):
        scene.time = (k + 0.5)/FPS
        scene.video.update()
        assert scene.video._read == k + 1
        assert np.array_equal(np.flipud(scene.video.texture.get_box().texture.read()), want[k]), f"source frame {k}"
    assert scene.video._stage.paths() == (count, 0)               # every frame on the segment path, none fell back


# ---- 6. two formats side by side ---------------------------------------------------------------------------------------------------------

def test_a_png_and_a_motion_jpeg_handle_keep_to_their_own(monkeypatch):
    """Each handle owns one decoder: frames landed alternately on a Motion-JPEG and a PNG handle are exact, each decoder counts its own
    frames only, the other format's paths entry answers (0, 0), and destroying one handle frees only its decoder's scratch"""
    import jpeg_ref as J
    from shaderflow_amd import mjpegsource, pngsource
    monkeypatch.delenv("SHADERFLOW_JPEG_SYNC", raising=False)
    monkeypatch.delenv("SHADERFLOW_PNG_SEGMENTS", raising=False)
    pictures = [D.mixed(37, 21, seed) for seed in range(4)]
    pngs = [P.encode(picture) for picture in pictures]
    assert pngs[0] == CASES["own-37x21"]["stream"]
    jpegs = [J.encode(J.picture("noise", 48, 32, seed), 90) for seed in range(3)]
    decoded = [mjpegsource.device_decode(stream, sync="auto") for stream in jpegs]      # the path a handle chooses, and its pixels
    subsequence = sum(1 for got in decoded if got["sync"]["subsequences"])
    headers = mjpegsource.parse_header(jpegs[0]), pngsource.parse_header(pngs[0])
    jpeg = Stage(headers[0], mjpegsource.capacity_for(headers[0], max(map(len, jpegs))), slots=1, codec=mjpegsource)
    png = Stage(headers[1], pngsource.capacity_for(headers[1], max(map(len, pngs))), slots=1)
    try:
        for k in range(3):
            jpeg.show(jpegs[k])
            png.show(pngs[k])
            assert np.array_equal(jpeg.read(), np.flipud(decoded[k]["rgb"])) and np.array_equal(png.read(), np.flipud(pictures[k])), k
        assert jpeg.paths("sfx_video_jpeg_paths") == (subsequence, 3 - subsequence) and png.paths() == (3, 0)
        assert jpeg.paths("sfx_video_png_paths") == (0, 0) and png.paths("sfx_video_jpeg_paths") == (0, 0)
        assert jpeg.bad() == (-1, 0) and png.bad() == (-1, 0)
    finally:
        jpeg.close()
    try:
        png.show(pngs[3])
        assert np.array_equal(png.read(), np.flipud(pictures[3]))
        assert png.bad() == (-1, 0) and png.paths() == (4, 0)
    finally:
        png.close()
