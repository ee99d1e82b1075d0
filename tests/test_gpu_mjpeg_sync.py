"""
Motion-JPEG entropy decoding with a lane per subsequence (csrc/jpeg_decode_kernels.hpp, 1b; csrc/capi_video_jpeg.hip) through the test entry
sfx_jpeg_decode_sync (`mjpegsource.device_decode(sync=…)`), against the lane-per-interval kernel (`sfx_jpeg_decode`), value for value:

  1. every stored stream and a Pillow-written one without restart markers, at subsequences of 8, 16 and 64 bytes with the production
     budget (255 rounds per phase): coefficients, status, pixels; no fall-back wherever tests/jpeg_sync_ref.py's Jacobi count is within
     the budget — all but long_420 at 8 bytes (293 rounds), which is exact all the same, with or without the fall-back;
  2. the fall-back itself (a budget of no rounds), the sampling modes and partial MCUs;
  3. damaged scans (the cases tests/test_gpu_mjpeg_in.py builds): a status where the lane-per-interval kernel has one, nothing drawn, and
     the next clean frame exact;
  4. a Pillow-written `.avi` through a ShaderVideo scene: SHADERFLOW_JPEG_SYNC=1 and =0 export the same bytes, in the frame loop and in
     the video sequence; and which path a frame takes by default.
"""
from __future__ import annotations

import functools
import io
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_ref as J  # noqa: E402
import jpeg_sync_ref as R  # noqa: E402
import test_gpu_mjpeg_in as T  # noqa: E402  (read, not edited: its damaged streams, its scene and its render)

pytestmark = pytest.mark.gpu

STREAMS = dict(R.golden_streams(), pillow_noise=R.pillow_noise())
BUDGET = 255                                                          # mjpegsource.SYNC_ROUNDS: the production budget


@functools.lru_cache(maxsize=None)
def serial(name: str) -> dict:
    """The lane-per-interval kernel's result, once per stream"""
    from shaderflow_amd.mjpegsource import device_decode
    got = device_decode(STREAMS[name])
    assert got["status"] == 0 and got["sync"] is None
    return got


@functools.lru_cache(maxsize=None)
def rounds(name: str, subsequence: int) -> int:
    if name in R.ROUNDS and subsequence in R.SIZES:
        return R.ROUNDS[name][R.SIZES.index(subsequence)]
    return R.decode(STREAMS[name], subsequence)["rounds"]


def test_the_budget_is_the_production_one_and_exempts_few():
    from shaderflow_amd import mjpegsource as M
    assert M.SYNC_ROUNDS == BUDGET and len(STREAMS) == 20
    for subsequence in R.SIZES:
        exempt = [name for name in STREAMS if rounds(name, subsequence) > BUDGET]
        print(f"{subsequence} bytes: not covered by {BUDGET} rounds: {exempt}")
        assert len(exempt) <= 2


@pytest.mark.parametrize("subsequence", R.SIZES)
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_the_subsequence_path_gives_the_interval_kernels_values(name, subsequence):
    from shaderflow_amd.mjpegsource import device_decode
    want = serial(name)
    got = device_decode(STREAMS[name], sync=True, subsequence_bytes=subsequence)
    sync = got["sync"]
    print(f"{name} at {subsequence} bytes: {sync}, the restatement needs {rounds(name, subsequence)} rounds")
    assert got["status"] == 0 and sync["subsequences"] > 1
    assert sync["subsequences"] == -(-len(R.Frame(STREAMS[name]).scan)//subsequence) + R.Frame(STREAMS[name]).intervals
    if rounds(name, subsequence) <= BUDGET:
        assert sync["fell_back"] == 0
    assert np.array_equal(got["coefficients"], want["coefficients"])
    assert np.array_equal(got["planes"], want["planes"]) and np.array_equal(got["rgb"], want["rgb"])


@pytest.mark.parametrize("name, subsequence", [("wide_420", 16), ("pillow_noise", 8), ("tall_444", 64)])
def test_without_rounds_the_interval_kernel_decodes(name, subsequence):
    from shaderflow_amd.mjpegsource import device_decode
    assert rounds(name, subsequence) > 0
    got = device_decode(STREAMS[name], sync=True, subsequence_bytes=subsequence, round_budget=0)
    assert got["sync"]["fell_back"] == 1 and got["sync"]["rounds_used"] == 0 and got["sync"]["subsequences"] > 1 and got["status"] == 0
    assert np.array_equal(got["coefficients"], serial(name)["coefficients"]) and np.array_equal(got["rgb"], serial(name)["rgb"])


def test_the_streams_cover_the_sampling_modes_and_partial_mcus():
    from shaderflow_amd.mjpegsource import parse_header
    headers = [parse_header(stream) for stream in STREAMS.values()]
    assert {(header.components, header.sampling) for header in headers} == {(3, (2, 2)), (3, (2, 1)), (3, (1, 1)), (1, (1, 1))}
    assert {(17, 9), (40, 24)} <= {(header.width, header.height) for header in headers}


@pytest.mark.parametrize("name, subsequence, budget", [("own_extremes", 2, 255), ("long_420", 128, None), ("pillow_noise", 256, 64), ("tall_420", 4096, None)])
def test_other_sizes_and_budgets(name, subsequence, budget):
    """Symbols longer than a subsequence (2 bytes), the production size, subsequences longer than the intervals"""
    from shaderflow_amd.mjpegsource import device_decode
    got = device_decode(STREAMS[name], sync=True, subsequence_bytes=subsequence, round_budget=budget)
    print(f"{name} at {subsequence} bytes: {got['sync']}, the restatement needs {rounds(name, subsequence)} rounds")
    assert got["status"] == 0 and np.array_equal(got["coefficients"], serial(name)["coefficients"])
    if rounds(name, subsequence) <= (BUDGET if budget is None else budget):
        assert got["sync"]["fell_back"] == 0


# ---- 3. damage ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("subsequence", [16, 128])
@pytest.mark.parametrize("case", ["truncated", "unassigned", "wrong-rst", "short-interval"])
def test_a_damaged_scan_has_a_status_on_either_path(case, subsequence):
    from shaderflow_amd.mjpegsource import device_decode
    stream, _, _ = T.damaged()[case]
    old = device_decode(stream)["status"]
    got = device_decode(stream, sync=True, subsequence_bytes=subsequence)
    print(f"{case} at {subsequence} bytes: status {old} from the interval kernel, {got['status']} from the subsequence path, {got['sync']}")
    assert old != 0 and got["status"] != 0
    assert not got["rgb"].any()                                        # a frame with a bad status is not drawn
    clean = device_decode(STREAMS["wide_420"], sync=True, subsequence_bytes=subsequence)
    assert clean["status"] == 0 and clean["sync"]["fell_back"] == 0 and np.array_equal(clean["coefficients"], serial("wide_420")["coefficients"])


# ---- 4. scenes, and the default rule -------------------------------------------------------------------------------------------------------

def pillow_clip(count: int, width: int = 64, height: int = 48) -> list:
    from PIL import Image
    out = []
    for seed in range(count):
        buffer = io.BytesIO()
        Image.fromarray(J.picture("noise", width, height, 20 + seed)).save(buffer, "JPEG", quality=90)
        out.append(buffer.getvalue())
    return out


def test_an_avi_without_restart_markers_plays_the_same_on_both_paths(monkeypatch, tmp_path):
    from shaderflow_amd.mjpeg import AviWriter
    from shaderflow_amd.mjpegsource import parse_header
    clip = pillow_clip(12)
    assert all(parse_header(frame).restart_interval == 0 for frame in clip)
    fd = os.open(tmp_path/"clip.avi", os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        writer = AviWriter(fd, 64, 48, T.FPS)
        writer.begin()
        for frame in clip:
            writer.add(frame)
        writer.finish()
    finally:
        os.close(fd)
    source = lambda: dict(path=tmp_path/"clip.avi")  # noqa: E731
    exports = {}
    for sequence in ("0", "1"):
        for path in ("0", "1"):
            monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", sequence)
            monkeypatch.setenv("SHADERFLOW_JPEG_SYNC", path)
            scene = T.video_scene(source)()
            exports[sequence, path] = T.render(scene, 12)
            assert (scene.video_sequence is not None) == (sequence == "1")
            if sequence == "0":
                sync, interval = scene.video._stage.paths()
                assert (sync > 0, interval > 0) == (path == "1", path == "0")
    assert len({frame.tobytes() for frame in exports["0", "0"]}) >= 10
    assert np.array_equal(exports["0", "1"], exports["0", "0"]) and np.array_equal(exports["1", "1"], exports["1", "0"])
    assert np.array_equal(exports["1", "0"], exports["0", "0"])


def test_the_default_rule(monkeypatch):
    from shaderflow_amd import mjpegsource as M
    monkeypatch.delenv("SHADERFLOW_JPEG_SYNC", raising=False)
    long, short = R.Frame(STREAMS["pillow_noise"]), R.Frame(STREAMS["tall_420"])
    assert long.intervals == 1 and long.scan_bytes >= M.SYNC_RULE*M.SYNC_SUBSEQUENCE
    assert short.scan_bytes//short.intervals < M.SYNC_RULE*M.SYNC_SUBSEQUENCE
    got = M.device_decode(STREAMS["pillow_noise"], sync="auto")
    assert got["sync"]["subsequences"] == -(-long.scan_bytes//M.SYNC_SUBSEQUENCE) + 1 and got["status"] == 0
    assert np.array_equal(got["coefficients"], serial("pillow_noise")["coefficients"])
    got = M.device_decode(STREAMS["tall_420"], sync="auto")
    assert got["sync"] == {"subsequences": 0, "rounds_used": 0, "fell_back": 0} and np.array_equal(got["coefficients"], serial("tall_420")["coefficients"])
    monkeypatch.setenv("SHADERFLOW_JPEG_SYNC", "1")
    assert M.device_decode(STREAMS["tall_420"], sync="auto")["sync"]["subsequences"] > 0
    monkeypatch.setenv("SHADERFLOW_JPEG_SYNC", "0")
    assert M.device_decode(STREAMS["pillow_noise"], sync="auto")["sync"]["subsequences"] == 0
