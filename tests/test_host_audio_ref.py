"""
tests/audio_ref.py — the float64 references and the bounds the STFT and filterbank kernels are held to (test_gpu_audio_shapes.py) —
against the oracle, on the CPU: the references and bounds are shown right before a GPU sees them.
"""
import numpy as np
import pytest

from oracle import binding as O
from tests import audio_ref as R


def test_constants_are_the_kernels():
    import re
    from pathlib import Path
    source = (Path(__file__).resolve().parent.parent/"shaderflow_amd"/"csrc"/"audio_kernels.hpp").read_text()
    assert int(re.search(r"constexpr int FILTERBANK_SPLITS = (\d+);", source).group(1)) == R.FILTERBANK_SPLITS
    assert R.STFT_K == R.STFT_K_MARGIN*R.STFT_K_MEASURED and R.STFT_K_MARGIN == 16
    assert R.TINY == 2.0**-149 and R.gamma(1) > R.U


@pytest.mark.parametrize("fft_n", R.FFT_NS)
def test_stft_ref_and_bound_against_the_oracles_transform(fft_n):
    """numpy's rfft on the oracle's window (stft_ref) and the oracle's radix-2 (O.fft_power): two independent float64 transforms, each
    rounded once to float32 — within stft_bound / amplitude_bound of each other at every shape the device is run at: mono, stereo and three
    channels, the three windows, the four signals, the five tells. Prints what the power lies beyond one ulp, in units of
    sqrt(want*peak): the figure STFT_K_MEASURED restates, sixteen times under STFT_K"""
    n = 1 << fft_n
    beyond = 0.0
    for channels in (1, 2, 3):
        for name, pcm in R.signals(channels, n).items():
            for window in R.WINDOWS:
                for tell in R.tells(n):
                    want = R.stft_ref(pcm, int(tell), fft_n, window)
                    got = O.fft_power(pcm, int(tell), fft_n, window).astype(np.float64)
                    assert want.shape == got.shape == (channels, n//2 + 1)
                    assert (np.abs(got - want) <= R.stft_bound(want)).all(), (channels, name, window, int(tell), R.worst_ratio(got, want, R.stft_bound(want)))
                    beyond = max(beyond, R.stft_excess(got, want))
                    want = R.stft_ref(pcm, int(tell), fft_n, window, "amplitude")
                    got = O.fft_power(pcm, int(tell), fft_n, window, amplitude=True).astype(np.float64)
                    assert (np.abs(got - want) <= R.amplitude_bound(want)).all(), (channels, name, window, int(tell), R.worst_ratio(got, want, R.amplitude_bound(want)))
                    if name == "silence":
                        assert not got.any() and not want.any()
                    spectrum = R.stft_ref(pcm, int(tell), fft_n, window, "complex")
                    assert spectrum.dtype == np.complex128 and np.array_equal(spectrum.real**2 + spectrum.imag**2, R.stft_ref(pcm, int(tell), fft_n, window))
    print(f"fft_n {fft_n}: the oracle's power lies {beyond:.2e}*sqrt(want*peak) beyond one ulp of numpy's (STFT_K_MEASURED {R.STFT_K_MEASURED:.2e})")
    assert beyond <= R.STFT_K_MEASURED*2                               # (another libm may move the figure; the margin is for the device)


def test_stream_frame_reads_zeros_on_both_sides():
    pcm = np.arange(1, 11, dtype=np.float32).reshape(1, 10)
    assert R.stream_frame(pcm, 1, 4).tolist() == [[0, 0, 0, 0]]                # tell - n - 1 … tell - 2 = -4 … -1
    assert R.stream_frame(pcm, 4, 4).tolist() == [[0, 1, 2, 3]]                # -1 … 2: the newest sample (index tell - 1) stays out
    assert R.stream_frame(pcm, 10, 4).tolist() == [[6, 7, 8, 9]]
    assert R.stream_frame(pcm, 13, 4).tolist() == [[9, 10, 0, 0]]
    assert R.stream_frame(pcm, 99, 4).tolist() == [[0, 0, 0, 0]]
    for n in (16, 4096):
        tells, total = R.tells(n), R.stream_total(n)
        assert tells[0] == 1 and tells[3] == total and tells[4] - 2 >= total and tells[4] - n - 1 < total      # the last frame hangs over the end


@pytest.mark.parametrize("fft_n,fft_size", R.RESAMPLED)
def test_resampled_input_is_the_oracles_converter(fft_n, fft_size):
    """resampled_input (the kernel's taps in numpy) against the oracle's sample-by-sample restatement of libsamplerate's linear converter,
    bit for bit, at the start of the stream, inside it and past its end; no size is a power of two (the DFT kernel's)"""
    n, ratio = 1 << fft_n, fft_size/(1 << fft_n)
    assert fft_size & (fft_size - 1) and fft_size % 2 == 0
    for channels in (1, 2):
        for name, pcm in R.signals(channels, n).items():
            for tell in R.tells(n):
                got = R.resampled_input(pcm, int(tell), fft_n, ratio, fft_size)
                frame = R.stream_frame(pcm, int(tell), n)
                want = np.stack([O.resample_linear(channel, ratio, fft_size) for channel in frame])
                assert got.dtype == np.float32 and np.array_equal(got, want), (channels, name, int(tell))
                power = R.resampled_ref(pcm, int(tell), fft_n, fft_size, 0)
                assert power.shape == (channels, fft_size//2 + 1) and (name != "silence" or not power.any())


CSR_SHAPES = [(kind, fft_bins, bins) for kind in R.KINDS for fft_bins, bins in ((9, 1), (9, 7), (17, 9), (33, 33), (2049, 65))]


@pytest.mark.parametrize("kind,fft_bins,bins", CSR_SHAPES)
def test_filterbank_ref_bound_and_float32_loop_against_the_oracle(kind, fft_bins, bins):
    """O.csr_dot (scipy's order in C) equals the numpy float32 loop bit for bit and lies within filterbank_bound of the float64 product —
    for every kind of matrix the device gets, repeated columns (both sum them) and rows without entries (exactly 0) included"""
    indptr, indices, data = R.csr_matrix(kind, bins, fft_bins)
    assert len(indptr) == bins + 1 and indptr[-1] == len(indices) == len(data) and (kind == "g") == (len(data) == 0)
    assert (indices >= 0).all() and (indices < fft_bins).all()
    rng = np.random.default_rng(bins)
    power = (rng.standard_normal((3, fft_bins))**2*rng.choice([1e-9, 1.0, 300.0], (3, 1))).astype(np.float32)
    got = O.csr_dot(indptr, indices, data, power)
    assert np.array_equal(got, R.csr_loop_f32(indptr, indices, data, power))
    want, size, n = R.filterbank_ref(indptr, indices, data, power)
    assert (np.abs(got - want) <= R.filterbank_bound(size, n)).all(), R.worst_ratio(got, want, R.filterbank_bound(size, n))
    assert not got[n == 0].any() and not want[n == 0].any()
    if kind != "g" and n[-1]:
        assert (n > 0).any() and indices.max() == fft_bins - 1        # the last fft bin is used: at 33 it is alone in its 32-chunk
    if kind == "b" and bins >= 64:
        assert not n[32:64].any() and n[64] and not n[5] and n[4]
    if kind == "c":
        assert n.max() == fft_bins
    if kind == "d":
        assert any((np.diff(indices[indptr[r]:indptr[r + 1]]) < 0).any() for r in range(bins))
    if kind == "e":
        assert (data < 0).any() and (data > 0).any()
    if kind == "f":
        repeated = [len(set(indices[indptr[r]:indptr[r + 1]].tolist())) < n[r] for r in range(bins)]
        assert all(repeated)
        # the float32 sum of a repeated column's weights, as the dense matrix of the MFMA path holds it, stays inside the same bound
        dense = np.zeros((bins, fft_bins), np.float32)
        for r in range(bins):
            for j in range(indptr[r], indptr[r + 1]):
                dense[r, indices[j]] += data[j]
        merged = dense.astype(np.float64) @ power.astype(np.float64).T
        assert (np.abs(merged - want) <= R.filterbank_bound(size, n)).all()
        last = np.zeros((bins, fft_bins), np.float32)               # what a dense build that ASSIGNS keeps: outside the bound
        for r in range(bins):
            for j in range(indptr[r], indptr[r + 1]):
                last[r, indices[j]] = data[j]
        assert (np.abs(last.astype(np.float64) @ power.astype(np.float64).T - want) > R.filterbank_bound(size, n)).any()


@pytest.mark.parametrize("fft_n", R.FFT_NS)
def test_exact_case_on_the_oracle(fft_n):
    """Window `none`, one impulse per channel of amplitude 1, 2 and -0.5: the oracle's float32 power is exactly 1, 4 and 0.25 in every bin
    of every frame that holds the impulses; with weights that are small integers over powers of two the float32 CSR product is the exact
    product — no order of summation can change a bit of it"""
    n = 1 << fft_n
    pcm, tells = R.exact_stream(3, n)
    assert len(tells) >= 12 and tells[0] - n - 1 == -2 and tells[-1] - 2 == n - 3 + n - 3      # from the first frame that holds all three to the last
    tells = tells[np.linspace(0, len(tells) - 1, 12).astype(int)]
    powers = np.stack([O.fft_power(pcm, int(tell), fft_n, 2) for tell in tells])
    assert np.array_equal(powers, np.broadcast_to(np.array([1.0, 4.0, 0.25], np.float32)[None, :, None], powers.shape))
    for bins in (7, 33):
        indptr, indices, data = R.exact_matrix(bins, n//2 + 1, seed=fft_n)
        counts = np.diff(indptr)
        assert counts.max() == n//2 + 1 and counts[3] == 0 and (data*8 == np.rint(data*8)).all() and np.abs(data).max() <= 8
        want, size, _ = R.filterbank_ref(indptr, indices, data, powers[0])
        assert size.max()*32 < 2**24 and (want*32 == np.rint(want*32)).all()       # multiples of 1/32 below 2**24 of them: exact in float32
        got = O.csr_dot(indptr, indices, data, powers[0])
        assert np.array_equal(got.astype(np.float64), want) and np.abs(want).max() > 0
