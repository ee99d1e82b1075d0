"""
The sound track of a Motion-JPEG AVI export on the device: `scene.main(output="clip.avi", pixel_format="mjpeg", sound_track=True)` through
the frame loop, the frame tape and the tape loop — the read-out ring's writer thread puts each frame's share of the PCM behind the frame
(sfx_ring_side_track) — against the same export without the track and the definition in shaderflow_amd/mjpeg.py (tests/avi_ref.py
parses and restates; tests/test_host_avi_audio.py holds the writer to it without a GPU).
"""
import ctypes as C
import struct

import numpy as np
import pytest

from shaderflow_amd import _native as N
from shaderflow_amd import mjpeg
from tests import avi_ref as A

pytestmark = pytest.mark.gpu

RATE = 44100
_clip: dict = {}


def clip() -> np.ndarray:
    """synth.sweep_clip(1.5, 44100), made once and never changed"""
    from shaderflow_amd import synth
    if "clip" not in _clip:
        _clip["clip"] = synth.sweep_clip(1.5, RATE)
        _clip["clip"].setflags(write=False)
    return _clip["clip"]


def scene_of(name):
    from examples.scenes import Basic, MusicBars, Visualizer, make
    from shaderflow_amd import synth
    if name == "basic":
        return make(Basic)
    if name == "bars":
        return make(MusicBars, audio=(clip(), RATE))
    if name == "mono":
        return make(MusicBars, audio=(np.ascontiguousarray(clip()[:, :1]), RATE))
    if name == "two":                                                   # a second module with a clip of its own, 0.1 s long
        class Two(MusicBars):
            audio_source = (clip(), RATE)

            def build(self):
                from shaderflow_amd.audio import ShaderAudio
                super().build()
                self.second = ShaderAudio(scene=self, name="iSecond").load(samples=clip()[:4410], samplerate=RATE)
        return Two()
    if name == "counting":                                              # tests/test_gpu_mjpeg.py's: an update() of its own puts it on the tape loop
        class Counting(Visualizer):
            audio_source = (clip(), RATE)
            background = synth.background_image(160, 90, seed=3)
            counted = 0

            def update(self):
                self.counted += 1
        return Counting()
    raise ValueError(name)


def export(name, output, batch, frames=30, fps=30.0, **kwargs):
    scene = scene_of(name)
    return scene, scene.main(width=96, height=64, fps=fps, ssaa=1.0, time=frames/fps, output=output, batch=batch, pixel_format="mjpeg", **kwargs)


def shares(frames: int, fps, channels: int, total: int) -> list:
    return [2*channels*(A.a(k + 1, RATE, fps, total) - A.a(k, RATE, fps, total)) for k in range(frames)]


@pytest.mark.parametrize("name,batch", [("bars", False), ("bars", True), ("counting", None)], ids=["frame-loop", "frame-tape", "tape-loop"])
def test_the_three_loops_carry_the_track(name, batch, tmp_path):
    """30 frames at 30 fps beside a 1.5 s clip: the video payloads are those of the same export without the track, byte for byte; the
    audio is the quantised clip's first second; `00dc` then `01wb` frame by frame and idx1 as the chunks lie (avi_ref.parse); both
    stream headers field by field; and decode_audio gives the track back (the round trip)"""
    from shaderflow_amd.audio.reader import decode_audio
    from tests.test_host_mjpeg import parse_avi
    _, silent = export(name, tmp_path/"silent.avi", batch)
    scene, path = export(name, tmp_path/"sound.avi", batch, sound_track=True)
    assert path == tmp_path/"sound.avi"
    if name == "counting":
        assert scene.tape_loop is not None and scene.tape_loop.frames_mirrored == 30 and scene.counted == 30
    want = [payload for _, payload in parse_avi(silent.read_bytes())["frames"]]
    avi = A.parse(path.read_bytes())
    assert len(want) == 30 and A.video(avi) == want
    pcm = mjpeg.pcm_s16(clip())
    assert A.audio(avi) == pcm[:RATE].tobytes() == A.s16(clip()[:RATE]).tobytes()
    assert A.order(avi) == [4*1470]*30 and [fourcc for fourcc, _, _ in avi["chunks"]] == [b"00dc", b"01wb"]*30
    A.check_streams(avi, 96, 64, 30, 30, 2, RATE, RATE)
    got, rate = decode_audio(path)
    assert rate == RATE and got.dtype == np.float32 and np.array_equal(got, pcm[:RATE].astype(np.float32)/np.float32(32768))


def test_a_clip_shorter_than_the_video_ends(tmp_path):
    """24 fps, 48 frames, the 1.5 s clip: 1837.5 sample frames a frame, the audio ends at 66 150 with frame 35 and frames 36 to 47 are
    `00dc` alone"""
    _, silent = export("bars", tmp_path/"silent.avi", True, frames=48, fps=24.0)
    _, path = export("bars", tmp_path/"sound.avi", True, frames=48, fps=24.0, sound_track=True)
    avi = A.parse(path.read_bytes())
    assert A.video(avi) == A.video(A.parse(silent.read_bytes())) and len(A.video(avi)) == 48
    assert A.order(avi) == shares(48, 24, 2, 66150) == [4*1837, 4*1838]*18 + [0]*12
    assert A.audio(avi) == A.s16(clip()).tobytes() and len(A.audio(avi)) == 4*66150
    A.check_streams(avi, 96, 64, 24, 48, 2, RATE, 66150)


def test_a_mono_clip_writes_one_channel(tmp_path):
    """A mono clip leaves the tape for the frame loop, and the track goes with it: one channel, nBlockAlign 2"""
    from shaderflow_amd.audio.reader import decode_audio
    scene, path = export("mono", tmp_path/"mono.avi", None, sound_track=True)
    avi = A.parse(path.read_bytes())
    assert scene.tape_loop is None and len(A.video(avi)) == 30
    assert struct.unpack("<HHIIHH", avi["streams"][1]["strf"]) == (1, 1, RATE, 2*RATE, 2, 16)
    assert A.order(avi) == [2*1470]*30 and A.audio(avi) == A.s16(clip()[:RATE, :1]).tobytes()
    A.check_streams(avi, 96, 64, 30, 30, 1, RATE, RATE)
    got, rate = decode_audio(path)
    assert rate == RATE and got.shape == (RATE, 1) and np.array_equal(mjpeg.pcm_s16(got), mjpeg.pcm_s16(clip()[:RATE, :1]))


def test_the_module_can_be_named(tmp_path):
    """`sound_track=` the module or its name is the same file as True when the scene has one; a name the scene has not raises"""
    _, first = export("bars", tmp_path/"true.avi", False, frames=4, sound_track=True)
    _, named = export("bars", tmp_path/"named.avi", False, frames=4, sound_track="iAudio")
    scene = scene_of("bars")
    scene.initialize()                                                  # build() makes the modules
    given = scene.main(width=96, height=64, fps=30.0, ssaa=1.0, time=4/30.0, output=tmp_path/"given.avi", batch=False, pixel_format="mjpeg", sound_track=scene.audio)
    assert first.read_bytes() == named.read_bytes() == given.read_bytes()
    with pytest.raises(ValueError, match="no audio module 'iOther'"):
        export("bars", tmp_path/"other.avi", False, frames=4, sound_track="iOther")
    kw = dict(width=96, height=64, fps=30.0, ssaa=1.0, time=4/30.0, batch=False, pixel_format="mjpeg")
    with pytest.raises(ValueError, match="'iAudio', 'iSecond'"):
        scene_of("two").main(output=tmp_path/"two.avi", sound_track=True, **kw)
    second = A.parse(scene_of("two").main(output=tmp_path/"second.avi", sound_track="iSecond", **kw).read_bytes())
    assert A.audio(second) == A.s16(clip()[:4410]).tobytes() and A.order(second) == [4*1470]*3 + [0]


def test_the_refusals_come_before_the_first_frame(tmp_path, monkeypatch):
    """A sink that cannot hold the track, or a scene without a clip: ValueError naming the `.avi` requirement (and, off the mjpeg path,
    the ffmpeg hook), with no ring made, no sink opened and no file left"""
    from shaderflow_amd.exporting import ExportingHelper
    made = []
    for method in ("make_buffers", "popen"):
        monkeypatch.setattr(ExportingHelper, method, lambda self, *args, _name=method, **kwargs: made.append(_name))
    with pytest.raises(ValueError, match=r"sound_track.*\.avi"):
        export("bars", "pipe", False, sound_track=True)
    with pytest.raises(ValueError, match=r"sound_track.*\.avi"):
        export("bars", tmp_path/"clip.mjpeg", False, sound_track=True)
    with pytest.raises(ValueError, match=r"sound_track.*\.avi.*ffhook"):
        scene_of("bars").main(width=96, height=64, fps=30.0, ssaa=1.0, time=1.0, output=tmp_path/"clip.avi", batch=False, pixel_format="yuv420p", sound_track=True)
    with pytest.raises(ValueError, match="no audio module"):
        export("basic", tmp_path/"basic.avi", False, sound_track=True)
    assert not made and not list(tmp_path.iterdir())


def test_the_ring_by_hand(tmp_path):
    """A sized framing-1 ring of three slots, five 16 x 16 sink frames from sfx_jpeg_encode of which the third (noise at quality 100) says
    it did not fit, and a five-entry side track with shares of 7, 5, 8, 1 and 19 bytes: the file holds `00dc` and `01wb` for frames 0,
    1, 3 and 4 and nothing for 2 or of its share; SFX_E_TOO_LARGE comes once, naming frame 2; sfx_ring_sizes is the four video sizes.
    A sixth frame is beyond the table, and a track cannot be set on an unsized ring, an unframed one, or one that has taken a frame."""
    import torch

    from tests import jpeg_ref as J
    from tests.test_gpu_mjpeg import device_encode
    context, lib = N.default_context(), N.lib()
    pictures = np.stack([J.picture(kind, 16, 16, seed=5) for kind in ("grey", "checker", "noise", "sparse", "checker")])
    _, _, raw = device_encode(pictures, 100, fits=False)
    headers = [struct.unpack("<III", frame[:12].tobytes()) for frame in raw]
    assert [h[0] for h in headers] == [0x504a4653]*5 and [h[2] == 0 for h in headers] == [True, True, False, True, True]
    capacity = raw.shape[1]
    payloads = [frame[64:64 + h[1]].tobytes() for frame, h in zip(raw, headers)]
    assert capacity == 64 + 768 and all(0 < h[1] <= 768 for k, h in enumerate(headers) if k != 2)
    side = np.random.default_rng(3).integers(0, 256, 40, dtype=np.uint8)
    ends = np.array([7, 12, 20, 21, 40], np.uint64)
    track = (lambda ring, table=ends: lib.sfx_ring_side_track(ring, side.ctypes.data, side.nbytes, N.as_ptr(table, C.c_uint64), len(table)))
    ring = N.Handle()
    N.check(lib.sfx_ring_create_sized(context.handle, capacity, 3, 1, C.byref(ring)))
    try:
        for bad in (np.array([7, 5], np.uint64), np.array([7, 41], np.uint64)):      # backwards; past the bytes
            assert track(ring, bad) == -1
        N.check(track(ring))
        device = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
        torch.cuda.synchronize()
        with open(tmp_path/"out.bin", "wb") as file:
            N.check(lib.sfx_ring_pipe_frames(ring, C.c_void_p(device.data_ptr()), capacity, 3, 0, -1, file.fileno()))
            with pytest.raises(N.NativeError, match="frame 2 does not fit") as caught:
                N.check(lib.sfx_ring_pipe_sync(ring, -1))
            assert caught.value.code == N.E_TOO_LARGE
            N.check(lib.sfx_ring_pipe_sync(ring, -1))                   # once
            N.check(lib.sfx_ring_pipe_frames(ring, C.c_void_p(device.data_ptr() + 3*capacity), capacity, 2, 0, -1, file.fileno()))
            N.check(lib.sfx_ring_pipe_sync(ring, -1))
            assert track(ring) == -1                                    # it has taken frames
            assert lib.sfx_ring_read_device_async(ring, C.c_void_p(device.data_ptr()), 2) == -1      # a sixth frame: the table has five entries
            assert b"side track has 5 entries" in lib.sfx_last_error()
            N.check(lib.sfx_ring_pipe_sync(ring, -1))
        shares_of = {0: side[0:7], 1: side[7:12], 3: side[20:21], 4: side[21:40]}
        want = b"".join(mjpeg.chunk(payloads[k]) + mjpeg.audio_chunk(shares_of[k].tobytes()) for k in (0, 1, 3, 4))
        assert (tmp_path/"out.bin").read_bytes() == want
        count, sizes = C.c_size_t(), (C.c_uint32*8)()
        N.check(lib.sfx_ring_sizes(ring, sizes, 8, C.byref(count)))
        assert list(sizes[:count.value]) == [len(payloads[k]) for k in (0, 1, 3, 4)]
    finally:
        N.check(lib.sfx_ring_destroy(ring))
    for create in (lambda out: lib.sfx_ring_create(context.handle, capacity, 3, out), lambda out: lib.sfx_ring_create_sized(context.handle, capacity, 3, 0, out)):
        other = N.Handle()
        N.check(create(C.byref(other)))
        try:
            assert track(other) == -1 and b"sized ring with framing 1" in lib.sfx_last_error()
        finally:
            N.check(lib.sfx_ring_destroy(other))
