"""
Pins tests/loudness_ref.py — the summation order of the two loudness targets — to numpy itself and to the reference's captured targets
(pipeline.npz), and shows that the windows the device test runs tell that order from the one the kernel had before. CPU only.
"""
import numpy as np
import pytest

from tests import loudness_ref as L
from tests.helpers import i16_to_f32


def reference_cut(stream: np.ndarray, tell: int, n: int) -> np.ndarray:
    """The window as the reference cuts it (audio/module.py:140, 457-458): the ring after `tell` samples have been rolled in, its last n
    columns without the newest — a strided column slice of a larger float32 array"""
    ring = np.zeros((stream.shape[0], stream.shape[1] + n + 8), np.float32)
    if tell:
        ring[:, -tell:] = stream[:, :tell]
    return ring[:, -(n + 1):-1]


def numpy_targets(window: np.ndarray):
    return 2*np.sqrt(np.mean(np.square(window)))*(2**0.5), np.std(window)


def case_windows(channels, n):
    stream = L.case_stream(channels, n)
    return [reference_cut(stream, tell, n) for tell in L.case_tells(n, stream.shape[1])], stream


def test_numpy_buffer_size():
    """The runs are numpy's buffered iterator's: if this fails numpy has moved, and the restatement, the kernel and the oracle follow it"""
    assert np.getbufsize() == L.RUN == 8192


@pytest.mark.parametrize("channels,n", L.CASES)
def test_restatement_equals_numpy(channels, n):
    windows, stream = case_windows(channels, n)
    assert stream.shape == (channels, 2*n + 2000) and stream.dtype == np.float32
    for window, tell in zip(windows, L.case_tells(n, stream.shape[1])):
        assert not window.flags.c_contiguous or channels == 1
        assert np.array_equal(window, L.stream_window(stream, tell, n))
        want, got = numpy_targets(window), L.targets(window)
        assert all(type(v) is np.float32 for v in (*want, *got))
        assert got[0] == want[0] and got[1] == want[1], (tell, got, want)
    assert L.case_tells(n, stream.shape[1])[3] % 8 and L.case_tells(n, stream.shape[1])[4] == stream.shape[1]


def test_restatement_equals_the_captured_targets(golden):
    """100 frames of the reference's own run: both columns, every frame"""
    g = golden("pipeline")
    stream = np.ascontiguousarray(i16_to_f32(g["pcm_i16"]).T)
    got = np.array([L.targets(L.stream_window(stream, int(tell), 4410)) for tell in g["tell"]])
    assert len(got) == 100
    assert got.dtype == np.float32                                  # (the fixture holds the float32 targets as the float64 a DynamicNumber stores)
    assert np.array_equal(got[:, 0].astype(np.float64), g["vol_target"])
    assert np.array_equal(got[:, 1].astype(np.float64), g["std_target"])
    # the order before: one pairwise sum over everything, the mean row by row — 84 of 100 frames
    parent = np.array([L.parent_targets(L.stream_window(stream, int(tell), 4410)) for tell in g["tell"]])
    assert int((parent[:, 0].astype(np.float64) == g["vol_target"]).sum()) == 84
    assert int((parent[:, 1].astype(np.float64) == g["std_target"]).sum()) == 84


@pytest.mark.parametrize("channels,n", L.CASES)
def test_windows_tell_the_orders_apart(channels, n):
    """A condition on the INPUTS of test_gpu_audio.py::test_volume_std_equals_numpy: wherever the two orders can differ, at least one of the
    case's windows gives different bits under the earlier order, so that test fails on a kernel that still sums that way. Elsewhere the
    orders are the same additions, and every window must agree."""
    windows, _ = case_windows(channels, n)
    differing = sum(L.parent_targets(w) != L.targets(w) for w in windows)
    if (channels, n) in L.DISCRIMINATING:
        assert differing >= 1
    else:
        assert differing == 0
    assert L.orders_differ(channels, n) == (channels*n > 8192 or (channels == 2 and n not in (1, 128, 136, 800, 4096)))
