"""
OpenDML exports on the device: `scene.main(output="clip.avi", pixel_format="mjpeg" | "png", opendml=bytes)` through the frame loop, the
frame tape and the tape loop — the read-out ring's writer thread leaves the gap in front of a segment's first frame (sfx_ring_segments) —
against the same export without the argument, the rule (`mjpeg.segment_cuts`) and the independent parser (tests/odml_ref.py); the
segmented files played back through a second scene; the ring by hand; the refusals; and the default, which is the file it was.
tests/test_host_opendml.py holds the writer, the layout and the readers without a GPU.
"""
import ctypes as C
import struct

import numpy as np
import pytest

from shaderflow_amd import _native as N
from shaderflow_amd import mjpeg
from tests import avi_ref as A
from tests import odml_ref as O

pytestmark = pytest.mark.gpu

W, H, FRAMES, FPS, RATE = 96, 64, 24, 30.0, 44100


def scene_of(name):
    """The small export scenes of tests/test_gpu_mjpeg.py and tests/test_gpu_png.py"""
    from tests.test_gpu_mjpeg import scene_of as make
    return make(name)


def export(name, output, batch, **kwargs):
    scene = scene_of(name)
    return scene, scene.main(width=W, height=H, fps=FPS, ssaa=1.0, time=FRAMES/FPS, output=output, batch=batch, **kwargs)


@pytest.fixture
def helpers(monkeypatch):
    """The ExportingHelper of every export made in the test, as it is when finish() returns"""
    from shaderflow_amd.exporting import ExportingHelper
    seen, finish = [], ExportingHelper.finish

    def spy(self):
        seen.append(self)
        return finish(self)
    monkeypatch.setattr(ExportingHelper, "finish", spy)
    return seen


def runs_of(sizes, sound):
    return [8 + size + (size & 1) + ((8 + share + (share & 1)) if share else 0) for size, share in zip(sizes, sound)]


@pytest.mark.parametrize("name,batch", [("bars", False), ("bars", True), ("counting", None)], ids=["frame-loop", "frame-tape", "tape-loop"])
@pytest.mark.parametrize("pixel_format", ["mjpeg", "png"])
def test_every_loop_and_both_codecs(pixel_format, name, batch, tmp_path, helpers):
    """24 frames with the sound track: first the AVI 1.0 export, then the same with budgets taken from that export's own chunk sizes —
    a cut exactly at a fit boundary (frames 0 to 2 and the headers are the budget to the byte: the gap goes in front of frame 3), the
    same less one byte (in front of frame 2), and a frame per segment. odml_ref validates the files; the payloads and the audio bytes
    are the AVI 1.0 export's; the gaps the ring's writer left are where the rule puts them."""
    scene, plain = export(name, tmp_path/"plain.avi", batch, pixel_format=pixel_format, sound_track=True)
    if name == "counting":
        assert scene.tape_loop is not None and scene.tape_loop.frames_mirrored == FRAMES
    old = A.parse(plain.read_bytes())
    assert helpers[-1]._cuts == [] and not any(word in plain.read_bytes() for word in (b"indx", b"odml", b"AVIX"))
    sizes, sound = [len(payload) for payload in A.video(old)], A.order(old)
    assert len(sizes) == FRAMES and sound == [4*1470]*FRAMES
    runs = runs_of(sizes, sound)
    start = len(mjpeg.AviWriter(None, W, H, FPS, track=mjpeg.SoundTrack(np.zeros((8, 2)), RATE), opendml=True).headers(0, 0, 0, 0))
    fit = start + sum(runs[:3])
    for tag, budget, first in (("fit", fit, 3), ("less", fit - 1, 2), ("each", min(runs) - 1, 1)):
        _, path = export(name, tmp_path/f"{tag}.avi", batch, pixel_format=pixel_format, sound_track=True, opendml=budget)
        data = path.read_bytes()
        avi = O.parse(data)
        cuts = mjpeg.segment_cuts(runs, start, budget)
        assert cuts[0] == first and (tag != "each" or cuts == list(range(1, FRAMES)))
        assert helpers[-1]._cuts == cuts and helpers[-1]._sizes == sizes          # sfx_ring_segment_cuts, sfx_ring_sizes
        assert avi["movis"][0] + 4 == start and len(avi["riffs"]) == len(cuts) + 1
        bounds = [0, *cuts, FRAMES]
        assert [len(mine) for mine in avi["per_segment"][b"00dc"]] == [b - a for a, b in zip(bounds[:-1], bounds[1:])]
        assert O.payloads(data, avi["walk"][b"00dc"]) == A.video(old)
        assert O.payloads(data, avi["walk"][b"01wb"]) == [payload for fourcc, _, payload in old["chunks"] if fourcc == b"01wb"]
        assert all(span <= budget for span in O.spans(avi)[:-1]) or tag == "each"
        assert avi["streams"][0]["strh"] == old["streams"][0]["strh"] and avi["streams"][1]["strh"] == old["streams"][1]["strh"]
        assert avi["streams"][0]["strf"] == old["streams"][0]["strf"] and avi["streams"][0]["strh"]["handler"] == {"mjpeg": b"MJPG", "png": b"MPNG"}[pixel_format]
        assert avi["total"] == FRAMES and avi["avih"][4] == first


def test_true_is_one_gibibyte_and_a_small_export_is_one_riff_chunk(tmp_path, helpers):
    _, plain = export("bars", tmp_path/"plain.avi", True, pixel_format="mjpeg")
    _, path = export("bars", tmp_path/"clip.avi", True, pixel_format="mjpeg", opendml=True)
    assert helpers[-1]._budget == 1 << 30 and helpers[-1]._cuts == []
    data = path.read_bytes()
    avi = O.parse(data)
    assert len(avi["riffs"]) == 1 and len(avi["streams"]) == 1 and b"AVIX" not in data and b"idx1" not in data
    assert O.payloads(data, avi["walk"][b"00dc"]) == A.video(A.parse(plain.read_bytes()))


# ---- the round trip ------------------------------------------------------------------------------------------------------------------

def back_scene(path, audio=True):
    from shaderflow_amd.audio import ShaderAudio
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo

    class Back(ShaderScene):
        def build(self):
            if audio:
                self.audio = ShaderAudio(scene=self, name="iAudio")
                self.audio.file = path                                  # the same file's PCM track
            self.video = ShaderVideo(scene=self, path=path)
            self.shader.fragment = "video"
    return Back()


def textures(path, count):
    """The file's frames, one by one, as the video plays them into its texture (top row first), and the track ShaderAudio read from it"""
    scene = back_scene(path)
    scene.main(width=W, height=H, fps=FPS, time=1/FPS, output=bytes)   # (its one frame is drawn at time 0: nothing is read yet)
    assert scene.video._read == 0 and scene.video.fps == FPS
    found = []
    for k in range(count):
        scene.time = (k + 0.5)/FPS
        scene.video.update()
        assert scene.video._read == k + 1
        found.append(np.flipud(scene.video.texture.get_box().texture.read()).copy())
    return scene.video.format, np.stack(found), np.array(scene.audio._file_reader.samples)


def played(path, monkeypatch, sequence):
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1" if sequence else "0")
    scene = back_scene(path, audio=False)
    raw = scene.main(width=W, height=H, fps=FPS, time=FRAMES/FPS, output=bytes)
    assert (scene.video_sequence is not None) == sequence
    return np.frombuffer(raw, np.uint8).reshape(FRAMES, H, W, 3)


@pytest.mark.parametrize("pixel_format", ["png", "mjpeg"])
def test_a_segmented_export_played_back(pixel_format, tmp_path, monkeypatch):
    """Several segments (three frames' worth of budget), played back by a second scene. png: at the video texture every frame is the first
    scene's rgb24 frame. mjpeg: every frame is the one the unsegmented twin plays — the same streams through the same decoder. Both: the
    native video sequence and the frame loop draw the same pictures from the segmented file as from its twin, and ShaderAudio(file=)
    reads the twin's track."""
    _, raw = export("bars", bytes, True)
    want = np.frombuffer(raw, np.uint8).reshape(FRAMES, H, W, 3)[:, ::-1]
    _, twin = export("bars", tmp_path/"twin.avi", True, pixel_format=pixel_format, sound_track=True)
    old = A.parse(twin.read_bytes())
    budget = 3*max(runs_of([len(p) for p in A.video(old)], A.order(old)))
    _, path = export("bars", tmp_path/"clip.avi", True, pixel_format=pixel_format, sound_track=True, opendml=budget)
    assert len(O.parse(path.read_bytes())["riffs"]) >= 8
    kind, got, track = textures(path, FRAMES)
    twin_kind, twin_got, twin_track = textures(twin, FRAMES)
    assert kind == twin_kind == pixel_format and np.array_equal(got, twin_got)
    if pixel_format == "png":
        assert np.array_equal(got, want)
    assert track.shape == (RATE*FRAMES//30, 2) and np.array_equal(track, twin_track)
    for sequence in (True, False):
        assert np.array_equal(played(path, monkeypatch, sequence), played(twin, monkeypatch, sequence)), sequence


# ---- the ring by hand, and the refusals ------------------------------------------------------------------------------------------------

def test_the_ring_by_hand(tmp_path):
    """tests/test_gpu_avi_audio.py's ring — three slots, five 16 x 16 sink frames of which the third says it did not fit, a side track —
    with segments from byte 100 and a budget that the second written frame already passes: the gaps are 24 zero bytes in front of the
    frames the rule names, the frame that is not written does not count, and sfx_ring_segment_cuts says where they went. Segments
    cannot be set on an unsized ring, an unframed one, one that has taken a frame, with budget 0 or with a gap above 64 bytes."""
    import torch

    from tests import jpeg_ref as J
    from tests.test_gpu_mjpeg import device_encode
    context, lib = N.default_context(), N.lib()
    pictures = np.stack([J.picture(kind, 16, 16, seed=5) for kind in ("grey", "checker", "noise", "sparse", "checker")])
    _, _, raw = device_encode(pictures, 100, fits=False)
    headers = [struct.unpack("<III", frame[:12].tobytes()) for frame in raw]
    assert [h[2] == 0 for h in headers] == [True, True, False, True, True]
    capacity, written = raw.shape[1], (0, 1, 3, 4)
    payloads = [frame[64:64 + h[1]].tobytes() for frame, h in zip(raw, headers)]
    side = np.random.default_rng(3).integers(0, 256, 40, dtype=np.uint8)
    ends = np.array([7, 12, 20, 21, 40], np.uint64)
    shares = {0: side[0:7], 1: side[7:12], 3: side[20:21], 4: side[21:40]}
    pieces = [mjpeg.chunk(payloads[k]) + mjpeg.audio_chunk(shares[k].tobytes()) for k in written]
    runs = [len(piece) for piece in pieces]
    budget = 100 + runs[0] + runs[1] + runs[2] - 1                       # frames 0, 1 and 3 pass it by a byte: the gap goes in front of frame 3
    want_cuts = mjpeg.segment_cuts(runs, 100, budget)
    assert want_cuts == [2]
    ring = N.Handle()
    N.check(lib.sfx_ring_create_sized(context.handle, capacity, 3, 1, C.byref(ring)))
    try:
        N.check(lib.sfx_ring_side_track(ring, side.ctypes.data, side.nbytes, N.as_ptr(ends, C.c_uint64), len(ends)))
        assert lib.sfx_ring_segments(ring, 100, 0, 24) == -1 and b"budget" in lib.sfx_last_error()
        assert lib.sfx_ring_segments(ring, 100, budget, 65) == -1 and b"64" in lib.sfx_last_error()
        N.check(lib.sfx_ring_segments(ring, 100, budget, 24))
        device = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
        torch.cuda.synchronize()
        with open(tmp_path/"out.bin", "wb") as file:
            N.check(lib.sfx_ring_pipe_frames(ring, C.c_void_p(device.data_ptr()), capacity, 3, 0, -1, file.fileno()))
            with pytest.raises(N.NativeError, match="frame 2 does not fit"):
                N.check(lib.sfx_ring_pipe_sync(ring, -1))
            N.check(lib.sfx_ring_pipe_frames(ring, C.c_void_p(device.data_ptr() + 3*capacity), capacity, 2, 0, -1, file.fileno()))
            N.check(lib.sfx_ring_pipe_sync(ring, -1))
            assert lib.sfx_ring_segments(ring, 100, budget, 24) == -1 and b"taken" in lib.sfx_last_error()
        want = b"".join((b"\0"*24 if k in want_cuts else b"") + piece for k, piece in enumerate(pieces))
        assert (tmp_path/"out.bin").read_bytes() == want
        count, cuts = C.c_size_t(), (C.c_uint32*8)()
        N.check(lib.sfx_ring_segment_cuts(ring, None, 0, C.byref(count)))
        assert count.value == 1
        N.check(lib.sfx_ring_segment_cuts(ring, cuts, 8, C.byref(count)))
        assert list(cuts[:count.value]) == want_cuts
    finally:
        N.check(lib.sfx_ring_destroy(ring))
    for create in (lambda out: lib.sfx_ring_create(context.handle, capacity, 3, out), lambda out: lib.sfx_ring_create_sized(context.handle, capacity, 3, 0, out)):
        other = N.Handle()
        N.check(create(C.byref(other)))
        try:
            assert lib.sfx_ring_segments(other, 100, 4096, 24) == -1 and b"sized ring with framing 1" in lib.sfx_last_error()
        finally:
            N.check(lib.sfx_ring_destroy(other))


def test_the_refusals_come_before_the_first_frame(tmp_path, monkeypatch):
    """`opendml` with a sink that is no `.avi` file of an mjpeg or png export, or a segment size out of range: ValueError, with no ring
    made, no sink opened and no file left"""
    from shaderflow_amd.exporting import ExportingHelper
    made = []
    for method in ("make_buffers", "popen"):
        monkeypatch.setattr(ExportingHelper, method, lambda self, *args, _name=method, **kwargs: made.append(_name))
    for output, extra in (("pipe", dict(pixel_format="mjpeg")), (tmp_path/"clip.mjpeg", dict(pixel_format="mjpeg")), ("pipe", dict(pixel_format="png")),
                          (tmp_path/"clip.avi", dict(pixel_format="rgb24")), (tmp_path/"clip.avi", dict(pixel_format="yuv420p")), ("pipe", {})):
        with pytest.raises(ValueError, match=r"opendml.*\.avi"):
            export("bars", output, False, opendml=True, **extra)
    for size in (100, 4095, (1 << 31) + 1, 1.5):
        with pytest.raises(ValueError, match="opendml.*4096"):
            export("bars", tmp_path/"clip.avi", False, pixel_format="mjpeg", opendml=size)
    with pytest.raises(ValueError, match="opendml.*no output"):
        scene_of("bars").main(width=W, height=H, fps=FPS, time=4/FPS, freewheel=True, opendml=True)
    assert not made and not list(tmp_path.iterdir())


def test_the_default_is_untouched(tmp_path):
    """Without `opendml` (and with None or False) the file has no `indx`, `odml` or `AVIX` and parses as the AVI 1.0 file it was"""
    files = []
    for tag, extra in (("default", {}), ("none", dict(opendml=None)), ("false", dict(opendml=False))):
        _, path = export("bars", tmp_path/f"{tag}.avi", True, pixel_format="mjpeg", sound_track=True, **extra)
        files.append(path.read_bytes())
    assert files[0] == files[1] == files[2]
    assert not any(word in files[0] for word in (b"indx", b"odml", b"AVIX", b"ix00"))
    avi = A.parse(files[0])
    assert len(A.video(avi)) == FRAMES and b"idx1" in files[0]
    A.check_streams(avi, W, H, FPS, FRAMES, 2, RATE, RATE*FRAMES//30)
