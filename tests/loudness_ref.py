"""
The two loudness targets (audio/module.py:74-75, 457-458) restated in numpy float32 scalars, one addition at a time, in the order
numpy 2.x takes for `np.mean` / `np.std` of a float32 window: the flat, channel-major sequence is cut into runs of `np.getbufsize()`
elements (its buffered iterator), every run is summed pairwise, and the runs are added in order to a float32 zero. Written from
numpy's observed results; tests/test_host_loudness.py holds it to `np.mean` / `np.std` themselves and to pipeline.npz.

csrc/audio_kernels.hpp (k_volume_std) and oracle/sfo_audio.c (sfo_volume_std) are the two implementations of this order.
"""
from __future__ import annotations

import numpy as np

F = np.float32
RUN = 8192                                                          # np.getbufsize() of an untouched numpy
SQRT2 = F(2**0.5)                                                   # the python float 2**0.5 meets a float32: rounded to float32


def pairwise(a) -> np.float32:
    """numpy's pairwise sum of float32 values: fewer than 8 one after another, up to 128 with eight accumulators, longer runs split
    at n/2 rounded down to a multiple of 8 and the halves added"""
    n = len(a)
    if n < 8:
        res = F(0)
        for v in a:
            res = F(res + v)
        return res
    if n <= 128:
        r = np.array(a[:8], F)                                      # eight accumulators: an elementwise add, no order of its own
        i = 8
        while i < n - n % 8:
            r = r + a[i:i + 8]
            i += 8
        res = F(F(F(r[0] + r[1]) + F(r[2] + r[3])) + F(F(r[4] + r[5]) + F(r[6] + r[7])))
        for v in a[i:]:
            res = F(res + v)
        return res
    half = n//2
    half -= half % 8
    return F(pairwise(a[:half]) + pairwise(a[half:]))


def buffered_sum(a) -> np.float32:
    """f32(0) plus the pairwise sum of each run of 8192 values, in order"""
    total = F(0)
    for first in range(0, len(a), RUN):
        total = F(total + pairwise(a[first:first + RUN]))
    return total


def _finish(x, mean, total_of) -> tuple[np.float32, np.float32]:
    count = F(len(x))
    volume = F(F(F(2)*np.sqrt(F(total_of(x*x)/count)))*SQRT2)
    d = x - mean
    return volume, np.sqrt(F(total_of(d*d)/count))


def targets(window: np.ndarray) -> tuple[np.float32, np.float32]:
    """(volume target, std target) of the (channels, n) float32 window"""
    x = np.ascontiguousarray(window, F).ravel()
    return _finish(x, F(buffered_sum(x)/F(len(x))), buffered_sum)


def parent_targets(window: np.ndarray) -> tuple[np.float32, np.float32]:
    """The order the kernel and the oracle had before they followed numpy's runs: mean(x²) and the variance each ONE pairwise sum over
    all values, the mean the channels' pairwise sums added in row order. Kept only so that tests can show they tell the two apart."""
    w = np.ascontiguousarray(window, F)
    x = w.ravel()
    total = F(0)
    for row in w:
        total = F(total + pairwise(row))
    return _finish(x, F(total/F(len(x))), pairwise)


def stream_window(planar: np.ndarray, tell: int, n: int) -> np.ndarray:
    """stream[tell-n-1 … tell-2] of every channel of the (channels, total) stream, zeros before its start: the ring's last n samples
    without the newest one (audio/module.py:140) once `tell` samples have been read"""
    out = np.zeros((planar.shape[0], n), F)
    first = tell - n - 1
    lo = max(first, 0)
    if first + n > lo:
        out[:, lo - first:] = planar[:, lo:first + n]
    return out


# ---- the shapes the kernel and the oracle are held to (test_host_loudness.py on numpy, test_gpu_audio.py on the device) -------------
# channels x window samples: the under-8 leaf; leaf boundary and first split; 8 kHz; a stereo count exactly at and just past one run of
# 8192; 44.1, 48 and 96 kHz (mono 9600 crosses a run); 18 runs
WINDOWS = (1, 5, 7, 64, 128, 129, 136, 800, 4096, 4097, 4410, 4800, 9600)
CASES = tuple((channels, n) for n in WINDOWS for channels in (1, 2)) + ((2, 70000),)
# Where the two orders can differ at all: more than one run, or two rows whose boundary is no node of the flat sequence's tree. Two rows
# of one sample are the same two additions either way; and with n a multiple of 8 and 128 < 2n <= 8192 the flat tree's first split falls
# exactly between the rows (n/2 of 2n, already a multiple of 8), so the row order IS the flat order: (2, 128), (2, 136), (2, 800), (2, 4096).
def orders_differ(channels: int, n: int) -> bool:
    return channels*n > RUN or (channels == 2 and n > 1 and not (2*n > 128 and n % 8 == 0))


DISCRIMINATING = tuple(case for case in CASES if orders_differ(*case))
# seeds at which parent_targets differs from targets in at least one of the case's windows (the first such seed counting up from 0;
# test_host_loudness.py asserts it); every other case takes seed 0
SEEDS = {(2, 7): 4, (2, 64): 2, (2, 129): 1, (1, 9600): 1, (2, 9600): 1}


def case_tells(n: int, total: int) -> list[int]:
    """1 and n//2: the window reaches before the stream and reads zeros; n + 1: its first sample is the stream's; mid-stream at no
    multiple of 8; the stream's end"""
    mid = n + 1003 + (1 if (n + 1003) % 8 == 0 else 0)
    return [1, n//2, n + 1, mid, total]


def case_stream(channels: int, n: int) -> np.ndarray:
    """(channels, 2n + 2000) float32: seeded noise with a small DC offset, so that the mean matters"""
    rng = np.random.default_rng(SEEDS.get((channels, n), 0))
    return (0.4*rng.standard_normal((channels, 2*n + 2000)) + 0.05).astype(F)
