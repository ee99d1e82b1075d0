"""
Motion-JPEG on the device (csrc/jpeg_kernels.hpp, capi_jpeg.hip, the sized read-out ring, scene.main(pixel_format="mjpeg")) against the
float64 restatement tests/jpeg_ref.py: the quantised coefficients, the entropy coder, the packed streams, batches, the ring that reads
frames of their own length, and whole exports.
"""
import io
import os
import struct

import numpy as np
import pytest

from shaderflow_amd import _native as N
from tests import jpeg_ref as J

pytestmark = pytest.mark.gpu


def device_encode(frames: np.ndarray, quality: int, bottom_up: bool = False, calls: int = 1, fits: bool = True):
    """frames (n, h, w, 3) as they lie on the device → (streams, the last frame's coefficients, the raw sink frames); `fits` False: the
    frames need not fit their sink frames (a 16 x 16 sink frame holds 768 bytes, 623 of them the header), no streams are returned"""
    import torch
    context = N.default_context()
    n, h, w = frames.shape[:3]
    encoder = N.JpegEncoder(context, w, h, quality)
    try:
        rgb = torch.from_numpy(np.array(frames)).cuda()                  # (a writable, contiguous copy)
        sink = torch.zeros(n*encoder.sink_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        per = n//calls
        for k in range(calls):
            encoder.encode(rgb.data_ptr() + k*per*h*w*3, sink.data_ptr() + k*per*encoder.sink_bytes, per, bottom_up)
        coefficients = encoder.coefficients().astype(np.int64)
        context.synchronize()
        raw = sink.cpu().numpy().reshape(n, -1)
        assert encoder.header() == J.header(w, h, quality)
    finally:
        encoder.destroy()
    streams = []
    for frame in (raw if fits else ()):
        magic, size, status = struct.unpack("<III", frame[:12].tobytes())
        assert magic == 0x504a4653 and status == 0 and 0 < size <= frame.size - 64, (magic, size, status)
        assert not frame[12:64].any()
        streams.append(frame[64:64 + size].tobytes())
    return streams, coefficients, raw


def pil_picture(stream: bytes) -> np.ndarray:
    Image = pytest.importorskip("PIL.Image")
    image = Image.open(io.BytesIO(stream))
    image.load()
    assert image.mode == "RGB"
    return np.asarray(image)


SIZES = [(16, 16), (48, 32), (40, 24), (17, 9), (1040, 16)]


@pytest.mark.parametrize("kind", ["gradient", "noise", "checker"])
@pytest.mark.parametrize("size", SIZES)
def test_coefficients_equal_the_restatement(size, kind):
    """Equal wherever the float64 value in front of the rounding is further than 1e-3 from a tie, at most 1 apart elsewhere, and the
    positions left out are at most 1 % (tests/test_host_mjpeg.py checks that on the CPU for the same inputs)"""
    w, h = size
    picture = J.picture(kind, w, h, seed=J.NOISE_SEEDS[size])
    for quality in (50, 90, 100):
        want, near_tie = J.coefficients(picture, quality), J.tie_distance(picture, quality) <= 1e-3
        assert near_tie.mean() <= 0.01
        for bottom_up in (False, True):
            stored = picture[::-1] if bottom_up else picture
            _, got, _ = device_encode(stored[None], quality, bottom_up, fits=False)
            assert got.shape == want.shape
            apart = np.abs(got - want)
            print(f"{kind} {w}x{h} q{quality} bottom_up={bottom_up}: {int((apart != 0).sum())} of {apart.size} differ, {int(near_tie.sum())} near a tie")
            assert not apart[~near_tie].any(), (size, kind, quality, bottom_up, np.argwhere((apart != 0) & ~near_tie)[:5])
            assert apart.max() <= 1


ENTROPY_CASES = [("grey", 48, 32, 90), ("extremes", 64, 48, 100), ("sparse", 48, 48, 25), ("gradient", 24, 272, 90)]
_entropy: dict = {}


def entropy_case(case):
    """(picture, the device's stream, its coefficients), encoded once per case"""
    if case not in _entropy:
        kind, w, h, quality = case
        picture = J.picture(kind, w, h, seed=5)
        streams, coefficients, _ = device_encode(picture[None], quality)
        _entropy[case] = (picture, streams[0], coefficients)
    return _entropy[case]


@pytest.mark.parametrize("case", ENTROPY_CASES, ids=lambda c: c[0])
def test_entropy_coder_is_lossless(case):
    """The device's stream, decoded by the restatement's decoder, gives exactly the device's own coefficients — and is, byte for byte,
    what the restatement's coder makes of them. Flat grey (EOB only), noise at quality 100 with a black and a white block in front (a
    stuffed FF 00, an 11-bit DC difference: noise alone has no such difference), isolated high-frequency terms at quality 25 (ZRL), and
    17 restart intervals (RSTn wraps past 7)."""
    kind, w, h, quality = case
    picture, stream, coefficients = entropy_case(case)
    decoded = J.decode(stream)
    assert (decoded["width"], decoded["height"], decoded["restart_interval"]) == (w, h, (w + 15)//16)
    assert decoded["length"] == len(stream)
    assert np.array_equal(decoded["coefficients"], coefficients)
    stats: dict = {}
    assert J.encode_coefficients(coefficients, w, h, quality, stats) == stream
    assert decoded["restart_markers"] == [k % 8 for k in range((h + 15)//16 - 1)]
    data = stream[len(J.header(w, h, quality)):]
    if kind == "grey":
        assert not coefficients[..., 1:].any()
    if kind == "extremes":
        assert b"\xff\x00" in data and stats["dc_size"] == 11
    if kind == "sparse":
        reference: dict = {}
        J.encode(picture, quality, reference)
        assert reference["zrl"] > 0 and stats["zrl"] > 0
    if kind == "gradient":
        assert len(decoded["restart_markers"]) == 16


@pytest.mark.parametrize("case", ENTROPY_CASES, ids=lambda c: c[0])
def test_pil_opens_the_streams(case):
    """… and the decoded picture is as close to the source as the restatement's stream, within 0.05 dB (they differ in tie roundings)"""
    kind, w, h, quality = case
    picture, stream, _ = entropy_case(case)
    got, want = pil_picture(stream), pil_picture(J.encode(picture, quality))
    assert got.shape == picture.shape
    a, b = J.psnr(got, picture), J.psnr(want, picture)
    print(f"{kind}: PSNR {a:.3f} dB, the restatement's {b:.3f} dB")
    assert (a == b) or abs(a - b) <= 0.05


def test_a_batch_equals_frame_by_frame():
    frames = np.stack([J.picture(kind, 40, 24, seed=k) for k, kind in enumerate(["gradient", "noise", "checker", "noise", "sparse"])])
    _, _, batch = device_encode(frames, 90, calls=1)
    _, _, single = device_encode(frames, 90, calls=5)
    for k in range(5):
        size = struct.unpack("<I", batch[k][4:8].tobytes())[0]
        assert np.array_equal(batch[k][:64 + size], single[k][:64 + size]), k
        assert batch[k][64:64 + size].tobytes() == J.encode_coefficients(J.decode(batch[k][64:64 + size].tobytes())["coefficients"], 40, 24, 90)


def sink_frames(payloads, capacity, bad=()):
    frames = np.zeros((len(payloads), capacity), np.uint8)
    for k, payload in enumerate(payloads):
        frames[k, :12] = np.frombuffer(struct.pack("<III", 0x504a4653, 0 if k in bad else len(payload), 1 if k in bad else 0), np.uint8)
        if k not in bad:
            frames[k, 64:64 + len(payload)] = np.frombuffer(payload, np.uint8)
    return frames


@pytest.mark.parametrize("framing, slots", [pytest.param(0, 3, id="0"), pytest.param(1, 3, id="1"), pytest.param(0, 2, id="0-2slots"), pytest.param(1, 2, id="1-2slots"),
                                            pytest.param(0, 5, id="0-5slots"), pytest.param(1, 5, id="1-5slots")])
def test_sized_ring(framing, slots, tmp_path):
    """Seven sink frames of different payload lengths (one of length 1, one odd) through a sized ring of three slots (two lanes), of two
    (one lane) and of five (four lanes: a header read on every one) into a file: exact, in order, framed and padded as asked; the sizes
    agree; a frame whose status says overflow fails the wait with its number, once"""
    import ctypes as C

    import torch
    context = N.default_context()
    capacity = 64 + 768
    rng = np.random.default_rng(9)
    payloads = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1, 7, 100, 768, 33, 2, 500)]
    ring = N.Handle()
    N.check(N.lib().sfx_ring_create_sized(context.handle, capacity, slots, framing, C.byref(ring)))
    try:
        device = torch.from_numpy(sink_frames(payloads, capacity)).cuda()
        torch.cuda.synchronize()
        with open(tmp_path/"out.bin", "wb") as file:
            N.check(N.lib().sfx_ring_pipe_frames(ring, C.c_void_p(device.data_ptr()), capacity, len(payloads), 0, -1, file.fileno()))
            N.check(N.lib().sfx_ring_pipe_sync(ring, -1))
        want = b"".join(p if framing == 0 else b"00dc" + struct.pack("<I", len(p)) + p + b"\0"*(len(p) % 2) for p in payloads)
        assert (tmp_path/"out.bin").read_bytes() == want
        count = C.c_size_t()
        sizes = (C.c_uint32*16)()
        N.check(N.lib().sfx_ring_sizes(ring, sizes, 16, C.byref(count)))
        assert list(sizes[:count.value]) == [len(p) for p in payloads]
        if slots < 3:
            return      # (three frames in one call would take a slot twice, and that slot's wait may meet the unfit frame inside the call)
        # frames 7…9 of the ring, the middle one marked as not fitting
        device = torch.from_numpy(sink_frames(payloads[:3], capacity, bad=(1,))).cuda()
        torch.cuda.synchronize()
        with open(tmp_path/"more.bin", "wb") as file:
            N.check(N.lib().sfx_ring_pipe_frames(ring, C.c_void_p(device.data_ptr()), capacity, 3, 1, -1, file.fileno()))
            with pytest.raises(N.NativeError, match="frame 8 does not fit"):
                N.check(N.lib().sfx_ring_pipe_sync(ring, -1))
            N.check(N.lib().sfx_ring_pipe_sync(ring, -1))
            N.check(N.lib().sfx_ring_pipe_frames(ring, C.c_void_p(device.data_ptr()), capacity, 1, 0, -1, file.fileno()))
            N.check(N.lib().sfx_ring_pipe_sync(ring, -1))
        frame = (lambda p: p if framing == 0 else b"00dc" + struct.pack("<I", len(p)) + p + b"\0"*(len(p) % 2))
        assert (tmp_path/"more.bin").read_bytes() == frame(payloads[0]) + frame(payloads[2]) + frame(payloads[0])
    finally:
        N.check(N.lib().sfx_ring_destroy(ring))


# ---- whole exports ---------------------------------------------------------------------------------------------------------------------

FPS = 30.0


def scene_of(name):
    from examples.scenes import Basic, MotionBlur, MusicBars, Visualizer, make
    from shaderflow_amd import synth
    if name == "basic":
        return make(Basic)
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


def export(name, w, h, frames, output, batch, **kwargs):
    scene = scene_of(name)
    return scene, scene.main(width=w, height=h, fps=FPS, ssaa=1.0, time=frames/FPS, output=output, batch=batch, **kwargs)


def encoded_rgb_export(name, w, h, frames, batch, quality=90):
    """The scene's rgb24 export (rows bottom-up, as a "pipe" delivers them) and sfx_jpeg_encode of each of its frames"""
    _, raw = export(name, w, h, frames, bytes, batch)
    rgb = np.frombuffer(raw, np.uint8).reshape(frames, h, w, 3)
    streams, _, _ = device_encode(rgb, quality, bottom_up=True)
    return rgb[:, ::-1], streams


@pytest.mark.parametrize("batch", [False, True], ids=["frame-loop", "frame-tape"])
@pytest.mark.parametrize("name,w,h", [("basic", 64, 48), ("bars", 96, 64)])
def test_exports(name, w, h, batch, tmp_path):
    """`.avi`, `.mjpeg` and "pipe" through the frame loop and the frame tape: frame k is sfx_jpeg_encode of frame k of the same scene's
    rgb24 export, byte for byte; the AVI parses; the first and last frames open in PIL as close to the source as the restatement's"""
    from tests.test_host_mjpeg import parse_avi
    frames = 30
    top_down, want = encoded_rgb_export(name, w, h, frames, batch)
    _, piped = export(name, w, h, frames, "pipe", batch, pixel_format="mjpeg")
    assert piped == b"".join(want)
    scene, path = export(name, w, h, frames, tmp_path/"clip.mjpeg", batch, pixel_format="mjpeg", jpeg_quality=90)
    assert path == tmp_path/"clip.mjpeg" and path.read_bytes() == piped and scene.exporting
    _, path = export(name, w, h, frames, tmp_path/"clip.avi", batch, pixel_format="mjpeg")
    avi = parse_avi(path.read_bytes())
    assert [payload for _, payload in avi["frames"]] == want
    assert avi["avih"][4] == frames and avi["avih"][8:10] == (w, h) and avi["avih"][0] == round(1e6/FPS)
    scale, rate, _, length = struct.unpack("<IIII", avi["strh"][20:36])
    assert rate/scale == FPS and length == frames and avi["strh"][:8] == b"vidsMJPG"
    for k in (0, frames - 1):
        got, reference = J.psnr(pil_picture(want[k]), top_down[k]), J.psnr(pil_picture(J.encode(top_down[k], 90)), top_down[k])
        print(f"{name} frame {k}: PSNR {got:.3f} dB, the restatement's {reference:.3f} dB")
        assert got >= reference - 0.05


def test_a_tape_loop_scene_gives_its_frame_loops_bytes():
    """A scene with an update() of its own (it counts frames) runs on the tape loop with mjpeg and delivers the frame loop's bytes"""
    frames = 30
    loop, want = export("counting", 96, 64, frames, "pipe", False, pixel_format="mjpeg")
    scene, got = export("counting", 96, 64, frames, "pipe", None, pixel_format="mjpeg")
    assert scene.tape_loop is not None and scene.tape_loop.frames_mirrored == frames and scene.counted == loop.counted == frames
    assert got == want and got.count(b"\xff\xd8\xff\xe0") == frames


def test_the_native_sequences_step_aside(monkeypatch):
    """A clock-only scene with mjpeg is drawn frame by frame — no sfx_sequence_run — and its frames are the encoded rgb24 export's;
    a sharded mjpeg export and an unknown pixel format raise ValueError before any frame"""
    w, h, frames = 64, 48, 12
    _, want = encoded_rgb_export("blur", w, h, frames, None)
    lib, calls = N.lib(), []
    run = lib.sfx_sequence_run

    def spy(*args):
        calls.append(args)
        return run(*args)
    monkeypatch.setattr(lib, "sfx_sequence_run", spy)
    scene, got = export("blur", w, h, frames, "pipe", None, pixel_format="mjpeg")
    assert scene.clock_loop and not calls
    assert got == b"".join(want)
    _, raw = export("blur", w, h, frames, bytes, None)
    assert calls, "the rgb24 export of the same scene runs the native sequence"
    monkeypatch.setattr(lib, "sfx_sequence_run", run)
    with pytest.raises(ValueError, match="mjpeg"):
        export("blur", w, h, frames, "pipe", False, pixel_format="mjpeg", shard=(0, 2))
    with pytest.raises(ValueError, match="pixel_format 'nv12'.*'mjpeg'"):
        export("blur", w, h, frames, "pipe", None, pixel_format="nv12")
    with pytest.raises(ValueError, match=r"\.avi"):
        export("blur", w, h, frames, "clip.mp4", None, pixel_format="mjpeg")


NOISE_FRAGMENT = """
    void main() {
        GetCamera(iCamera);
        vec2 p = iCamera.gluv*977.0;
        vec3 seed = vec3(dot(p, vec2(12.9898, 78.233)), dot(p, vec2(39.346, 11.135)), dot(p, vec2(73.156, 52.235)));
        fragColor = vec4(fract(sin(seed)*43758.5453), 1);
    }
"""


def test_a_frame_that_does_not_fit_raises_and_the_context_goes_on():
    """Noise at quality 100 at 16 x 16: the restatement's own stream exceeds the sink frame's 768 bytes by more than a quarter (623 of them
    are the header). scene.main raises the RuntimeError, nothing faults, and the context renders a normal frame afterwards"""
    from examples.scenes import Basic, make

    class Noise(Basic):
        def build(self):
            super().build()
            self.shader.fragment = NOISE_FRAGMENT
    kw = dict(width=16, height=16, fps=FPS, ssaa=1.0, time=2/FPS, batch=False)
    rgb = np.frombuffer(make(Noise).main(output=bytes, **kw), np.uint8).reshape(2, 16, 16, 3)
    assert len(J.encode(rgb[0, ::-1], 100)) > 1.25*768
    with pytest.raises(RuntimeError, match="frame 0 does not fit at quality 100"):
        make(Noise).main(output="pipe", pixel_format="mjpeg", jpeg_quality=100, **kw)
    again = np.frombuffer(make(Noise).main(output=bytes, **kw), np.uint8).reshape(2, 16, 16, 3)
    assert np.array_equal(again, rgb)
    _, ok = export("basic", 64, 48, 2, "pipe", False, pixel_format="mjpeg")
    assert ok.count(b"\xff\xd9") >= 2
