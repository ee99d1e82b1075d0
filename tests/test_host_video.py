"""
The host side of the video sequence (shaderflow_amd/video.py, shaderflow_amd/videosequence.py), without a device:

  1. the native YUV4MPEG2 reader: header variants, the frames' bytes, what it refuses (by tag), a truncated last frame;
  2. `landing_frames` against a literal simulation of `ShaderVideo.update()`'s rule (reference: shaderflow/video.py:57-66) over the
     export's own clock.

`VideoSequence.applicable` needs built scenes, and building a scene makes device textures: those cases are in tests/test_gpu_video.py.
"""
from __future__ import annotations

import numpy as np
import pytest

from shaderflow_amd.scheduler import freewheel_clock
from shaderflow_amd.video import PlanarFile, parse_y4m_header
from shaderflow_amd.videosequence import landing_frames, slot_count

W, H = 64, 36
FRAME = W*H*3//2


def write_y4m(path, header: bytes, frames, frame_line: bytes = b"FRAME\n", tail: bytes = b""):
    with open(path, "wb") as file:
        file.write(header)
        for frame in frames:
            file.write(frame_line)
            file.write(np.asarray(frame, np.uint8).tobytes())
        file.write(tail)
    return path


def clip(count: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (count, FRAME), dtype=np.uint8)


# ---- 1. YUV4MPEG2 --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("header, fps", [
    (b"YUV4MPEG2 W64 H36 F30:1 Ip A1:1 C420jpeg\n", 30.0),
    (b"YUV4MPEG2 W64 H36 F25:1\n", 25.0),                                # no C tag: 4:2:0
    (b"YUV4MPEG2 W64 H36 F30000:1001 Ip C420mpeg2\n", 30000/1001),
    (b"YUV4MPEG2 W64 H36 F60:1 Ip A1:1 C420paldv XYSCSS=420JPEG XCOLORRANGE=LIMITED\n", 60.0),
    (b"YUV4MPEG2 H36 W64 C420 F24:1\n", 24.0),
])
def test_y4m_header_variants_and_frame_bytes(tmp_path, header, fps):
    frames = clip(4)
    reader = PlanarFile(write_y4m(tmp_path/"clip.y4m", header, frames))
    assert (reader.width, reader.height) == (W, H) and reader.fps == fps and reader.frame_bytes == FRAME
    got = list(reader)
    assert len(got) == 4
    for a, b in zip(got, frames):
        assert a.dtype == np.uint8 and a.shape == (FRAME,) and np.array_equal(a, b)


def test_y4m_readinto_fills_the_callers_buffer(tmp_path):
    frames = clip(3, seed=1)
    reader = PlanarFile(write_y4m(tmp_path/"clip.y4m", b"YUV4MPEG2 W64 H36 F30:1\n", frames, frame_line=b"FRAME Xanything\n"))
    buffer = np.zeros(FRAME, np.uint8)
    for frame in frames:
        assert reader.readinto(buffer) is True and np.array_equal(buffer, frame)
    assert reader.readinto(buffer) is False and reader.readinto(buffer) is False


@pytest.mark.parametrize("header, names", [
    (b"YUV4MPEG2 W64 H36 F30:1 C444\n", "C444"),
    (b"YUV4MPEG2 W64 H36 F30:1 C420p10\n", "C420p10"),
    (b"YUV4MPEG2 W64 H36 F30:1 Ii\n", "Ii"),
    (b"YUV4MPEG2 W64 H36 F30:1 C420jpeg XCOLORRANGE=FULL\n", "XCOLORRANGE=FULL"),
    (b"YUV4MPEG2 W63 H36 F30:1\n", "W63"),
    (b"YUV4MPEG2 W64 H35 F30:1\n", "H35"),
])
def test_y4m_refuses_what_it_does_not_read_and_names_the_tag(tmp_path, header, names):
    with pytest.raises(ValueError, match=names):
        parse_y4m_header(header)
    with pytest.raises(ValueError, match=names):
        PlanarFile(write_y4m(tmp_path/"clip.y4m", header, clip(1)))


def test_y4m_a_truncated_last_frame_ends_the_clip(tmp_path):
    frames = clip(3, seed=2)
    path = write_y4m(tmp_path/"clip.y4m", b"YUV4MPEG2 W64 H36 F30:1\n", frames, tail=b"FRAME\n" + frames[0].tobytes()[:FRAME//3])
    got = list(PlanarFile(path))
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, frames))


def test_y4m_a_broken_frame_line_is_an_error(tmp_path):
    path = write_y4m(tmp_path/"clip.y4m", b"YUV4MPEG2 W64 H36 F30:1\n", clip(2), frame_line=b"FRAMF\n")
    with pytest.raises(ValueError, match="FRAME"):
        list(PlanarFile(path))


def test_raw_planar_file_reads_whole_frames(tmp_path):
    frames = clip(3, seed=3)
    path = tmp_path/"clip.i420"
    path.write_bytes(frames.tobytes() + b"\x01"*17)                      # … and a short tail that is no frame
    reader = PlanarFile(path, W, H, 30.0)
    got = list(reader)
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, frames))


# ---- 2. the schedule -----------------------------------------------------------------------------------------------------------------

def simulate(times, fps, first_read, available):
    """ShaderVideo.update() frame by frame (video.py:57-66 there, video.py `update` here), literally: returns (landings, read, exhausted)"""
    read, exhausted, out = first_read, False, []
    for time in times:
        landed = -1
        if not exhausted and time > (read/fps):
            if available is not None and read >= available:
                exhausted = True                                     # StopIteration
            else:
                landed, read = read, read + 1
        out.append(landed)
    return out, read, exhausted


@pytest.mark.parametrize("scene_fps, clip_fps, speed, first_read, available", [
    (60.0, 20.0, 1.0, 0, None), (60.0, 30.0, 1.0, 0, None), (60.0, 60.0, 1.0, 0, None), (30.0, 60.0, 1.0, 0, None),
    (60.0, 29.97, 1.0, 0, None), (60.0, 30.0, 1.7, 0, None), (60.0, 30.0, 0.4, 0, None), (24.0, 25.0, 1.0, 0, None),
    (60.0, 30.0, 1.0, 0, 7), (60.0, 60.0, 1.0, 0, 1), (60.0, 60.0, 1.0, 0, 0), (60.0, 30.0, 1.0, 5, None), (60.0, 30.0, 1.0, 5, 9),
    (60.0, 30.0, 1.0, 9, 9), (60.0, 20.0, 2.5, 3, 40),
])
def test_landing_frames_is_update_walked_over_the_clock(scene_fps, clip_fps, speed, first_read, available):
    times, _, _ = freewheel_clock(scene_fps, 90, speed)
    want, read, _ = simulate(times, clip_fps, first_read, available)
    got = landing_frames(times, clip_fps, first_read, available)
    assert got.tolist() == want
    landed = got[got >= 0]
    assert landed.tolist() == list(range(first_read, read))             # in source order, none skipped, at most one per scene frame
    if available is None and clip_fps <= scene_fps/speed and not first_read:
        assert len(landed) >= int(90*speed*clip_fps/scene_fps) - 1      # the clip keeps up with its own rate


def test_landing_frames_masks_like_a_source_that_ends():
    """What the driver does when the reader learns the length late: landings of the endless schedule at or beyond the end are dropped"""
    times, _, _ = freewheel_clock(60.0, 60, 1.0)
    endless = landing_frames(times, 30.0)
    for available in (0, 1, 5, 29):
        masked = endless.copy()
        masked[masked >= available] = -1
        assert masked.tolist() == landing_frames(times, 30.0, 0, available).tolist()


def test_slots_are_bounded():
    assert slot_count(3840*2160*3) == 10 and slot_count(3840*2160*3)*3840*2160*3 <= 256 << 20
    assert slot_count(1920*1080*3) == 32 and slot_count(1 << 30) == 4
    assert all(slot_count(n) % 2 == 0 for n in (1, 12345, 6220800, 24883200, 1 << 29))
