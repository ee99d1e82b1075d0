"""
The subsequence path of Motion-JPEG entropy decoding (csrc/jpeg_decode_kernels.hpp, 1b) in its plain-Python restatement
(tests/jpeg_sync_ref.py): the speculative pass, the rounds, the scan and the write pass give tests/jpeg_ref.py's coefficients exactly.

Jacobi rounds to the fixed point, per stored stream, at subsequences of 8 / 16 / 64 bytes (jpeg_sync_ref.ROUNDS, held to the
restatement below; the GPU tests take from it which streams a round budget covers):

    long_420 293/191/39   long_grey 8/5/2      mid_420 75/34/9      mid_444 46/23/6     no_dht_420 85/42/10   odd_420 55/27/7
    odd_422 43/22/6       odd_grey 19/9/2      one_mcu_420 28/14/3  one_mcu_444 5/1/0   own_extremes 166/83/20 own_sparse 9/5/1
    partial_420 27/13/3   partial_422 19/9/3   partial_444 5/2/0    tall_420 30/15/4    tall_444 21/9/2       wide_420 85/42/10
    wide_422 15/9/2

The maxima are 293, 191 and 39. (The stored pictures are noise: blocks without an EOB, where a chain that starts inside a block learns the
zigzag index late. With the production budget of 255 rounds only long_420 at 8 bytes is not covered.)
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_decode_ref as D  # noqa: E402
import jpeg_ref as J  # noqa: E402
import jpeg_sync_ref as R  # noqa: E402

STREAMS = R.golden_streams()


def serial(stream: bytes) -> np.ndarray:
    coefficients = J.decode(D.with_tables(stream))["coefficients"]
    return coefficients.reshape(-1, *coefficients.shape[2:])


def exact(stream: bytes, subsequence: int) -> dict:
    got = R.decode(stream, subsequence)
    assert not got["errors"] and np.array_equal(got["coefficients"], serial(stream))
    return got


def test_the_table_covers_the_stored_streams():
    assert sorted(R.ROUNDS) == sorted(STREAMS) and len(STREAMS) == 19
    assert [max(rounds[k] for rounds in R.ROUNDS.values()) for k in range(3)] == [293, 191, 39]


@pytest.mark.parametrize("subsequence", R.SIZES)
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_the_coefficients_are_the_serial_decoders(name, subsequence):
    got = exact(STREAMS[name], subsequence)
    print(f"{name} at {subsequence} bytes: {got['subsequences']} subsequences, {got['rounds']} rounds")
    assert got["rounds"] == R.ROUNDS[name][R.SIZES.index(subsequence)]


@pytest.mark.parametrize("name", ["odd_grey", "partial_422", "mid_444", "wide_422"])
def test_the_chains_count_the_rounds_of_the_plain_loop(name):
    for subsequence in R.SIZES:
        frame = R.Frame(STREAMS[name])
        plain, merged = R.Sync(frame, subsequence), R.Sync(frame, subsequence)
        assert plain.jacobi() == merged.chains() == R.ROUNDS[name][R.SIZES.index(subsequence)]
        assert plain.entry == merged.entry and plain.settled()


@pytest.mark.parametrize("name", ["tall_420", "own_extremes", "mid_420", "long_grey"])
def test_a_budget_of_the_jacobi_count_settles_the_two_phases(name):
    """The device's rounds run inside workgroups, in two phases; a budget of the Jacobi count (below the workgroup's lanes) is enough"""
    for subsequence in R.SIZES:
        rounds = R.ROUNDS[name][R.SIZES.index(subsequence)]
        got = R.decode(STREAMS[name], subsequence, budget=rounds)
        assert rounds < R.GROUP and not got["fell_back"] and np.array_equal(got["coefficients"], serial(STREAMS[name]))
    assert R.decode(STREAMS[name], 8, budget=0)["fell_back"]


def test_a_stream_with_many_subsequences():
    from shaderflow_amd.mjpegsource import parse_header
    stream = R.pillow_noise()
    header = parse_header(stream)
    assert (header.width, header.height, header.restart_interval, header.sampling) == (128, 96, 0, (2, 2))
    for subsequence in R.SIZES:
        got = exact(stream, subsequence)
        print(f"pillow_noise at {subsequence} bytes: {got['subsequences']} subsequences, {got['rounds']} rounds")
        assert got["frame"].intervals == 1 and (subsequence != 8 or got["subsequences"] >= 3*R.GROUP)


# ---- boundary cases ----------------------------------------------------------------------------------------------------------------------

def test_a_stuffed_ff_straddles_a_cut():
    stream = STREAMS["long_420"]
    frame = R.Frame(stream)
    pairs = [n for n in range(len(frame.scan) - 1) if frame.scan[n] == 0xff and frame.scan[n + 1] == 0]
    assert pairs
    for subsequence in (8, 16, 64):
        straddling = [n for n in pairs if (n + 1) % subsequence == 0]
        if subsequence < 64:
            assert straddling                                          # (the 00 is a cut's byte: the cut moves one byte on)
        lanes = R.lanes_of(frame, subsequence)
        for n in straddling:
            assert any(lane is not None and lane[1] == n + 2 for lane in lanes) and not any(lane is not None and lane[1] == n + 1 for lane in lanes)
        exact(stream, subsequence)


def test_a_symbol_longer_than_a_subsequence_passes_through_a_lane():
    stream = STREAMS["own_extremes"]                                   # DC differences of 11 bits behind 9-bit codes: 20 bits
    frame = R.Frame(stream)
    sync = R.Sync(frame, 2)
    sync.chains()
    passed = [n for n, lane in enumerate(sync.lanes) if lane is not None and not lane[3] and sync.entry[n] is not None and sync.entry[n][0] >= lane[2]]
    assert passed and all(sync.result[n][0] == sync.entry[n] and sync.result[n][1] == 0 for n in passed)
    coefficients, errors = sync.write()
    assert not errors and np.array_equal(coefficients, serial(stream))


def test_intervals_shorter_than_a_subsequence():
    stream = STREAMS["own_sparse"]                                     # two intervals in 155 bytes
    got = exact(stream, 256)
    lanes = [lane for lane in R.lanes_of(got["frame"], 256) if lane is not None]
    assert got["frame"].intervals == 2 and len(lanes) == 2 and all(lane[3] and lane[4] for lane in lanes) and got["rounds"] == 0


def test_seventeen_intervals_wrap_the_restart_markers():
    stream = J.encode(J.picture("noise", 16, 16*17, 3), 90)           # an interval per MCU row: RST0 … RST7, RST0 … RST7
    info = J.decode(stream)
    assert info["restart_markers"] == [n % 8 for n in range(16)]
    for subsequence in R.SIZES:
        got = exact(stream, subsequence)
        assert got["frame"].intervals == 17
