"""
Lossless PNG on the device (csrc/png_kernels.hpp, capi_png.hip, scene.main(pixel_format="png")) against the restatement
tests/png_ref.py, byte for byte, through the C-ABI: the filtered stream, the code lengths, the packed files at the smallest shapes
where something can go wrong, batches, both row orders, and whole exports through the three loops. Lossless means array_equal.
"""
import io
import struct

import numpy as np
import pytest

from shaderflow_amd import _native as N
from tests import avi_ref as A
from tests import png_ref as P

pytestmark = pytest.mark.gpu

_reference: dict = {}


def reference(w, h, kind):
    """(picture, the restatement's file, its filtered stream), made once and never changed"""
    key = (w, h, kind)
    if key not in _reference:
        picture = P.picture(kind, w, h, seed=w*h)
        picture.setflags(write=False)
        _reference[key] = (picture, P.encode(picture), P.filter_rows(picture)[0])
    return _reference[key]


def device_encode(frames: np.ndarray, bottom_up: bool = False, calls: int = 1):
    """frames (n, h, w, 3) as they lie on the device → (the PNG files, the last frame's filtered stream)"""
    import torch
    context = N.default_context()
    n, h, w = frames.shape[:3]
    encoder = N.PngEncoder(context, w, h)
    try:
        assert encoder.sink_bytes == 64 + P.capacity(w, h)
        rgb = torch.from_numpy(np.array(frames)).cuda()
        sink = torch.zeros(n*encoder.sink_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        per = n//calls
        for k in range(calls):
            encoder.encode(rgb.data_ptr() + k*per*h*w*3, sink.data_ptr() + k*per*encoder.sink_bytes, per, bottom_up)
        filtered = encoder.filtered()
        context.synchronize()
        raw = sink.cpu().numpy().reshape(n, -1)
    finally:
        encoder.destroy()
    streams = []
    for frame in raw:
        magic, size, status = struct.unpack("<III", frame[:12].tobytes())
        assert magic == 0x504a4653 and status == 0 and 0 < size <= frame.size - 64, (magic, size, status)
        assert not frame[12:64].any()
        streams.append(frame[64:64 + size].tobytes())
    return streams, filtered


def pil_picture(stream: bytes) -> np.ndarray:
    Image = pytest.importorskip("PIL.Image")
    image = Image.open(io.BytesIO(stream))
    image.load()
    assert image.mode == "RGB"
    return np.asarray(image)


def first_difference(got: bytes, want: bytes) -> str:
    at = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} bytes, the restatement {len(want)}; first difference at byte {at}"


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("size", P.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_files_equal_the_restatement(size, kind):
    """1x1, 2x1, 3x5 (rows shorter than the filters reach, less than a stripe), 17x8 and 16x9 (one stripe, one stripe and a row), 130x67
    (a partial last stripe, rows that are no multiple of 16 bytes), 344x16 (a stripe's code leaves in several 1 KiB flushes) with
    zeros (runs past 258, a run across a flush), gradients along x, y and both (every filter type: tests/test_host_png.py), noise
    (the fixed codes) and rows of 0xFF: the filtered stream and the file are the restatement's, and Pillow decodes the source"""
    w, h = size
    picture, want, want_filtered = reference(w, h, kind)
    streams, filtered = device_encode(picture[None])
    assert np.array_equal(filtered[:, 0], want_filtered[:, 0]), "filter types"
    assert np.array_equal(filtered, want_filtered)
    assert streams[0] == want, first_difference(streams[0], want)
    assert np.array_equal(pil_picture(streams[0]), picture)


@pytest.mark.parametrize("size,kind", [((130, 67), "diagonal"), ((16, 9), "noise"), ((3, 5), "vertical")], ids=lambda v: str(v))
def test_bottom_up_reads_the_rows_in_reverse(size, kind):
    w, h = size
    picture, want, want_filtered = reference(w, h, kind)
    streams, filtered = device_encode(picture[None, ::-1], bottom_up=True)
    assert np.array_equal(filtered, want_filtered)
    assert streams[0] == want, first_difference(streams[0], want)
    flipped, _ = device_encode(picture[None, ::-1], bottom_up=False)
    assert flipped[0] == P.encode(picture[::-1]) and np.array_equal(pil_picture(flipped[0]), picture[::-1])


def test_a_batch_equals_frame_by_frame():
    """3 distinct frames in one call (grid.z = 3) and in three calls: the restatement's files each time; the filtered stream is the last frame's"""
    frames = np.stack([reference(130, 67, kind)[0] for kind in ("diagonal", "noise", "ff")])
    want = [reference(130, 67, kind)[1] for kind in ("diagonal", "noise", "ff")]
    batch, filtered = device_encode(frames, calls=1)
    single, _ = device_encode(frames, calls=3)
    assert len(set(want)) == 3 and batch == want and single == want
    assert np.array_equal(filtered, reference(130, 67, "ff")[2])


@pytest.mark.parametrize("name", ["fibonacci", "one-symbol", "no-match", "flat"])
def test_code_lengths_equal_the_restatement(name):
    counts = P.histograms()[name]
    want, want_fixed, _ = P.tables(counts)
    got, fixed = N.PngEncoder.code_lengths(N.default_context(), counts)
    assert np.array_equal(got, want) and fixed == want_fixed
    for part in (got[:P.LITERALS], got[P.LITERALS:]):
        assert sum(2.0**-int(v) for v in part if v) == 1.0 and part.max() <= 15


# ---- whole exports ---------------------------------------------------------------------------------------------------------------------

FPS = 30.0
W, H = 96, 64


def scene_of(name):
    from examples.scenes import MotionBlur, MusicBars, Visualizer, make
    from shaderflow_amd import synth
    if name == "bars":
        return make(MusicBars, audio=(synth.sweep_clip(1.5, 44100), 44100))
    if name == "blur":
        return make(MotionBlur, background=synth.background_image(160, 90, seed=4))
    if name == "counting":
        class Counting(Visualizer):
            audio_source = (synth.sweep_clip(1.5, 44100), 44100)
            background = synth.background_image(160, 90, seed=3)
            counted = 0

            def update(self):
                self.counted += 1
        return Counting()
    raise ValueError(name)


def export(name, frames, output, batch, **kwargs):
    scene = scene_of(name)
    return scene, scene.main(width=W, height=H, fps=FPS, ssaa=1.0, time=frames/FPS, output=output, batch=batch, **kwargs)


def split(piped: bytes) -> list:
    """PNG files back to back → the files"""
    files, at = [], 0
    while at < len(piped):
        _, size = P.chunks(piped[at:])
        files.append(piped[at:at + size])
        at += size
    return files


def check_frames(files: list, rgb: np.ndarray) -> None:
    """Every file is the restatement's of the rgb24 export's frame (rows bottom-up there) and decodes to exactly it"""
    assert len(files) == len(rgb)
    for k, (file, frame) in enumerate(zip(files, rgb)):
        assert np.array_equal(pil_picture(file), frame[::-1]), k
    for k in (0, len(rgb) - 1):
        assert files[k] == P.encode(rgb[k, ::-1]), k


def test_the_three_loops_give_the_same_lossless_frames():
    """The `counting` scene (an update() of its own) through the frame loop, the frame tape's gathered batches and the tape loop: the
    same bytes, and each PNG decodes to exactly the rgb24 export's frame"""
    frames = 12
    _, raw = export("counting", frames, bytes, False)
    rgb = np.frombuffer(raw, np.uint8).reshape(frames, H, W, 3)
    loop, want = export("counting", frames, "pipe", False, pixel_format="png")
    check_frames(split(want), rgb)
    scene, got = export("counting", frames, "pipe", None, pixel_format="png")
    assert scene.tape_loop is not None and scene.tape_loop.frames_mirrored == frames and scene.counted == loop.counted == frames
    assert got == want


@pytest.mark.parametrize("batch", [False, True], ids=["frame-loop", "frame-tape"])
def test_bars_through_the_frame_loop_and_the_frame_tape(batch, tmp_path, monkeypatch):
    """`bars` (the tape's own scene class): "pipe" and `.avi` hold the same files, which decode to the rgb24 export of the same loop;
    SHADERFLOW_PIXEL_FORMAT=png asks for the same"""
    frames = 12
    _, raw = export("bars", frames, bytes, batch)
    rgb = np.frombuffer(raw, np.uint8).reshape(frames, H, W, 3)
    _, piped = export("bars", frames, "pipe", batch, pixel_format="png")
    files = split(piped)
    check_frames(files, rgb)
    monkeypatch.setenv("SHADERFLOW_PIXEL_FORMAT", "png")
    _, path = export("bars", frames, tmp_path/"clip.avi", batch)
    monkeypatch.delenv("SHADERFLOW_PIXEL_FORMAT")
    assert path == tmp_path/"clip.avi"
    avi = A.parse(path.read_bytes())
    assert A.video(avi) == files and len(avi["streams"]) == 1
    assert struct.unpack("<IiiHH4sIiiII", avi["streams"][0]["strf"]) == (40, W, H, 1, 24, b"MPNG", W*H*3, 0, 0, 0, 0)
    assert avi["streams"][0]["strh"]["handler"] == b"MPNG" and avi["avih"][4] == frames


def test_the_native_sequences_step_aside(monkeypatch):
    """A clock-only scene with png is drawn frame by frame — no sfx_sequence_run — and gives the rgb24 export's pictures"""
    frames = 12
    lib, calls = N.lib(), []
    run = lib.sfx_sequence_run

    def spy(*args):
        calls.append(args)
        return run(*args)
    monkeypatch.setattr(lib, "sfx_sequence_run", spy)
    scene, got = export("blur", frames, "pipe", None, pixel_format="png")
    assert scene.clock_loop and not calls
    _, raw = export("blur", frames, bytes, None)
    assert calls, "the rgb24 export of the same scene runs the native sequence"
    monkeypatch.setattr(lib, "sfx_sequence_run", run)
    check_frames(split(got), np.frombuffer(raw, np.uint8).reshape(frames, H, W, 3))


def test_avi_with_the_sound_track(tmp_path):
    """`.avi` with sound_track=True: video and audio parse (tests/avi_ref.py), the video payloads are the silent export's, the audio
    is the quantised clip's share, `00dc` then `01wb` frame by frame"""
    from shaderflow_amd import mjpeg, synth
    frames = 15
    _, silent = export("bars", frames, tmp_path/"silent.avi", True, pixel_format="png")
    _, path = export("bars", frames, tmp_path/"sound.avi", True, pixel_format="png", sound_track=True)
    avi = A.parse(path.read_bytes())
    assert A.video(avi) == A.video(A.parse(silent.read_bytes())) and len(A.video(avi)) == frames
    pcm = mjpeg.pcm_s16(synth.sweep_clip(1.5, 44100))
    assert A.audio(avi) == pcm[:1470*frames].tobytes()
    assert A.order(avi) == [4*1470]*frames and [fourcc for fourcc, _, _ in avi["chunks"]] == [b"00dc", b"01wb"]*frames
    picture, sound = avi["streams"]
    assert picture["strh"]["handler"] == b"MPNG" and picture["strf"][16:20] == b"MPNG"
    assert sound["strh"]["type"] == b"auds" and struct.unpack("<HHIIHH", sound["strf"]) == (1, 2, 44100, 44100*4, 4, 16)


def test_what_png_refuses(tmp_path):
    with pytest.raises(ValueError, match="'png' is not sharded"):
        export("blur", 4, "pipe", False, pixel_format="png", shard=(0, 2))
    with pytest.raises(ValueError, match=r"\.avi"):
        export("blur", 4, tmp_path/"clip.mp4", None, pixel_format="png")
    with pytest.raises(ValueError, match=r"sound_track.*\.avi"):
        export("bars", 4, "pipe", None, pixel_format="png", sound_track=True)
    with pytest.raises(ValueError, match="pixel_format 'nv12'.*'mjpeg'.*'png'"):
        export("blur", 4, "pipe", None, pixel_format="nv12")
