"""
The STFT and filterbank kernels (k_stft_power, k_dft_power, k_filterbank_csr, k_filterbank_mfma + k_filterbank_reduce) at the small, odd
and exact shapes test_gpu_audio.py does not reach, against tests/audio_ref.py: numpy's float64 rfft and a float64 product, with bounds
that are derived there (one float32 ulp plus the float64 transform's own error; gamma(n + splits)*S for the MFMA sums) and held to the
oracle on the CPU by test_host_audio_ref.py. Every bin and every value is asserted, none through allclose. Each test prints its worst
|error|/bound.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import _native as N
from tests import audio_ref as R
from tests.test_gpu_audio import Audio, gpu  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

WHATS = ("power", "amplitude", "complex")


def plan_of(audio: Audio, fft_n, window, csr, bins, fft_size=None) -> N.Handle:
    """An sfx_stft_plan, or with `fft_size` the resampled one (linear_resample_taps' positions, as ShaderSpectrogram.plan() passes them)"""
    if fft_size is None:
        return audio.plan(fft_n, window, *csr, bins)
    from shaderflow_amd.audio.spectrogram import linear_resample_taps
    a, b, w = (np.ascontiguousarray(t) for t in linear_resample_taps(1 << fft_n, fft_size/(1 << fft_n), fft_size))
    assert len(a) == fft_size
    indptr, indices, data = (np.ascontiguousarray(csr[0], np.int32), np.ascontiguousarray(csr[1], np.int32), np.ascontiguousarray(csr[2], np.float32))
    h = N.Handle()
    N.check(audio.lib.sfx_stft_plan_resampled(audio.gpu.ctx.handle, fft_n, fft_size, N.as_ptr(a, C.c_int32), N.as_ptr(b, C.c_int32), N.as_ptr(w, C.c_double),
                                              window, bins, audio.pcm.shape[1], N.as_ptr(indptr, C.c_int32), N.as_ptr(indices, C.c_int32),
                                              N.as_ptr(data, C.c_float), C.byref(h)))
    return h


def spectra(audio: Audio, plan, tells, fft_bins, what):
    """(frames, channels, fft_bins): float32 power or amplitude through sfx_stft_power, complex128 through sfx_stft_spectrum"""
    tells = np.ascontiguousarray(tells, np.int64)
    shape = (len(tells), audio.pcm.shape[1], fft_bins)
    if what == "complex":
        pairs = np.zeros(shape + (2,), np.float64)
        N.check(audio.lib.sfx_stft_spectrum(plan, audio.handle, N.as_ptr(tells, C.c_int64), len(tells), N.as_ptr(pairs, C.c_double)))
        return pairs[..., 0] + 1j*pairs[..., 1]
    N.check(audio.lib.sfx_stft_plan_magnitude(plan, int(what == "amplitude")))
    out = np.zeros(shape, np.float32)
    N.check(audio.lib.sfx_stft_power(plan, audio.handle, N.as_ptr(tells, C.c_int64), len(tells), N.as_ptr(out, C.c_float)))
    return out


BOUNDS = {"power": R.stft_bound, "amplitude": R.amplitude_bound, "complex": R.complex_bound}


def hold_spectra(gpu, channels, fft_n, window, fft_size=None):
    """The four signals, five tells each (start of the stream to half a window past its end), power, amplitude and the complex spectrum:
    every bin within its bound of the float64 reference; silence exactly 0. Returns the worst |error|/bound per output."""
    n = 1 << fft_n
    fft_bins = (fft_size or n)//2 + 1
    tells = R.tells(n)
    worst = dict.fromkeys(WHATS, 0.0)
    for name, pcm in R.signals(channels, n).items():
        audio = Audio(gpu, pcm.T)
        plan = plan_of(audio, fft_n, window, R.csr_matrix("a", 1, fft_bins), 1, fft_size)
        for what in WHATS:
            got = spectra(audio, plan, tells, fft_bins, what)
            if fft_size is None:
                want = np.stack([R.stft_ref(pcm, int(tell), fft_n, window, what) for tell in tells])
            else:
                want = np.stack([R.resampled_ref(pcm, int(tell), fft_n, fft_size, window, what) for tell in tells])
            assert got.shape == want.shape
            bound = BOUNDS[what](want)
            if what == "power":
                # derived, not fitted: stft_bound is first order in the transform's error e; |X + e|**2 also holds |e|**2 <= (STFT_K/2)**2*peak
                # (audio_ref.second_order). Without it the DFT sum missed the bound at two bins only: (4, 48) and (8, 768), impulses, window
                # `none`, bin N/3, where the spectrum of the resampled impulse is exactly 0 and the device gives 9.0e-32 and 6.4e-31 (peaks
                # 5.1 and 45.6) — the square of a float64 rounding error, which a plain sum in numpy gives to the digit
                bound = bound + R.second_order(want)
            error = np.abs(got - want)
            ratio = R.worst_ratio(got, want, bound)
            worst[what] = max(worst[what], ratio)
            assert (error <= bound).all(), (name, what, ratio, np.argwhere(error > bound)[:4].tolist())
            assert not got[0].any()                                   # tell = 1: the frame ends before the stream's first sample
            assert not got.any() if name == "silence" else (got[2].any(axis=-1).all() and got[3].any(axis=-1).all() and got[4].any(axis=-1).all())
        N.check(gpu.lib.sfx_stft_plan_destroy(plan))
        N.check(gpu.lib.sfx_audio_destroy(audio.handle))
    return worst


@pytest.mark.parametrize("window", R.WINDOWS)
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fft_n", R.FFT_NS)
def test_radix2_stft_at_every_size(gpu, fft_n, channels, window):
    """k_stft_power at every size the plan accepts: at fft_n 4 to 8 a block's 256 threads outnumber the N/2 packed points or the N/4
    butterflies and the bit reversal runs at its smallest logM; mono, stereo and three channels in the block index; frames whose window
    lies before the stream's start and hangs over its end. The bound is one float32 ulp plus the float64 transform's error
    (audio_ref.stft_bound): a wrong twiddle at one stage, a lost half-sample or a float32 intermediate is outside it."""
    worst = hold_spectra(gpu, channels, fft_n, window)
    print(f"fft_n {fft_n} x {channels}, window {window}: worst error/bound " + ", ".join(f"{what} {ratio:.3f}" for what, ratio in worst.items()))


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("fft_n,fft_size", R.RESAMPLED)
def test_dft_sum_at_small_sizes(gpu, fft_n, fft_size, channels):
    """k_dft_power (transform sizes that are no power of two, reached with sample_rateio 1.5 and 3): 13 to 769 bins — fewer than a
    block's threads, more than them — over inputs resampled by the plan's taps, all three windows, against the same rfft within the same
    bound"""
    for window in R.WINDOWS:
        worst = hold_spectra(gpu, channels, fft_n, window, fft_size)
        print(f"fft_n {fft_n} -> {fft_size} x {channels}, window {window}: worst error/bound " + ", ".join(f"{what} {ratio:.3f}" for what, ratio in worst.items()))


# ---- filterbank ----------------------------------------------------------------------------------------------------------------------
# (kind of matrix, fft_n, bins, channels, frames): fft_bins 9, 17, 33 (one real column in the last 32-chunk) and 2 049; bins below,
# at and above one row tile and no multiple of 8; frames*channels = 1, 31, 32, 33 and 65 columns (a last column tile that is whole,
# partial, a single column); mono, stereo and three channels in the col / channels output index. Bands of one or two 32-chunks
# (fewer than FILTERBANK_SPLITS) at fft_n 4 to 6, of all 65 under a dense row at 12.
FILTERBANK_CASES = [
    ("a", 12, 65, 2, 16), ("a", 12, 33, 3, 11), ("a", 6, 31, 1, 31), ("a", 5, 9, 1, 65), ("a", 4, 7, 1, 1), ("a", 4, 1, 3, 11), ("a", 6, 8, 2, 16), ("a", 5, 32, 1, 33),
    ("b", 12, 65, 3, 11), ("b", 6, 65, 1, 33),
    ("c", 12, 33, 1, 1), ("c", 12, 9, 2, 16), ("c", 6, 32, 1, 31), ("c", 4, 8, 3, 11),
    ("d", 12, 31, 1, 65), ("d", 5, 33, 2, 16),
    ("e", 12, 32, 2, 16), ("e", 6, 7, 3, 11),
    ("f", 12, 33, 2, 16), ("f", 4, 9, 1, 31), ("f", 6, 65, 3, 11),
    ("g", 5, 8, 1, 1), ("g", 12, 33, 2, 16),
]


def test_filterbank_cases_reach_every_edge():
    """(no device needed, but it belongs to the list above)"""
    cases = FILTERBANK_CASES
    assert {c[0] for c in cases} == set(R.KINDS) and {c[1] for c in cases} == {4, 5, 6, 12}
    assert {c[2] for c in cases} == {1, 7, 8, 9, 31, 32, 33, 65} and {c[3] for c in cases} == {1, 2, 3}
    assert {c[3]*c[4] for c in cases} == {1, 31, 32, 33, 65}


def columns_of(values):
    """(frames, channels, x) -> (frames*channels, x): column = frame*channels + channel"""
    return values.reshape(-1, values.shape[-1])


def targets_layout(product, frames, channels):
    """(bins, frames*channels) -> (frames, bins, channels), the layout of sfx_spectrogram_targets"""
    return product.reshape(product.shape[0], frames, channels).transpose(1, 0, 2)


@pytest.mark.parametrize("kind,fft_n,bins,channels,frames", FILTERBANK_CASES)
def test_filterbank_at_every_edge(gpu, kind, fft_n, bins, channels, frames):
    """Both filterbank kernels on matrices of the test's own over the device's own power spectra: the CSR result is the oracle's and the
    numpy float32 loop's, bit for bit; the MFMA result lies within gamma(n + FILTERBANK_SPLITS)*S of the float64 product row by row — a
    quiet row is held as tightly as a loud one; rows without entries are exactly 0 in both. Kind f (a column named more than once in a
    row) failed for MFMA while the dense matrix was built by assignment."""
    n = 1 << fft_n
    fft_bins = n//2 + 1
    rng = np.random.default_rng(fft_n*1000 + bins)
    total = R.stream_total(n)
    pcm = (0.4*rng.standard_normal((total, channels))).astype(np.float32)
    csr = R.csr_matrix(kind, bins, fft_bins)
    audio = Audio(gpu, pcm)
    plan = audio.plan(fft_n, 0, *csr, bins)
    tells = np.linspace(n//2, total + n//2, frames).astype(np.int64) if frames > 1 else np.array([total], np.int64)
    power = audio.power(plan, tells, fft_n)
    assert power.any(axis=2).all()
    flat = columns_of(power)
    assert flat.shape == (frames*channels, fft_bins)
    oracle = np.stack([O.csr_dot(*csr, p) for p in power])
    assert np.array_equal(oracle, targets_layout(R.csr_loop_f32(*csr, flat), frames, channels))
    got_csr = audio.targets(plan, tells, bins, mfma=False)
    assert np.array_equal(got_csr, oracle), np.argwhere(got_csr != oracle)[:4].tolist()
    want, size, count = R.filterbank_ref(*csr, flat)
    bound = targets_layout(R.filterbank_bound(size, count), frames, channels)
    want = targets_layout(want, frames, channels)
    got = audio.targets(plan, tells, bins, mfma=True)
    error = np.abs(got - want)
    ratio = R.worst_ratio(got, want, bound)
    print(f"{kind} fft_n {fft_n}, {bins} bins, {channels} x {frames}: MFMA worst error/bound {ratio:.3f}, CSR {R.worst_ratio(got_csr, want, bound):.3f}")
    assert (error <= bound).all(), (ratio, np.argwhere(error > bound)[:4].tolist())
    empty = count == 0
    assert not got[:, empty].any() and not got_csr[:, empty].any()
    assert kind == "g" or (got[:, ~empty] != 0).all()
    N.check(gpu.lib.sfx_stft_plan_destroy(plan))
    N.check(gpu.lib.sfx_audio_destroy(audio.handle))


@pytest.mark.parametrize("fft_n,bins,channels,frames", [(4, 9, 3, 11), (5, 7, 2, 16), (6, 33, 3, 11), (12, 65, 3, 11), (12, 32, 1, 33), (14, 8, 2, 1)])
def test_filterbank_exact_case_needs_no_tolerance(gpu, fft_n, bins, channels, frames):
    """Window `none` and one impulse per channel of amplitude 1, 2 and -0.5: the power is exactly 1, 4 and 0.25 in every bin — asserted of
    the device first. The weights are small integers over powers of two, so every partial sum of every row is exact in float32 whatever
    the order: MFMA equals CSR equals the exact product, bit for bit. A dropped term, a wrong even / odd lane mapping, a wrong accumulator
    row or a split taken twice is a different number."""
    n = 1 << fft_n
    fft_bins = n//2 + 1
    planar, tells = R.exact_stream(channels, n)
    tells = tells[np.linspace(0, len(tells) - 1, frames).astype(int)]
    csr = R.exact_matrix(bins, fft_bins, seed=fft_n)
    audio = Audio(gpu, planar.T)
    plan = audio.plan(fft_n, 2, *csr, bins)
    power = audio.power(plan, tells, fft_n)
    assert np.array_equal(power, np.broadcast_to((np.array(R.EXACT_AMPLITUDES[:channels], np.float32)**2)[None, :, None], power.shape))
    want, size, _ = R.filterbank_ref(*csr, columns_of(power))
    assert size.max()*32 < 2**24 and np.array_equal(want.astype(np.float32).astype(np.float64), want) and np.abs(want).max() > 0
    want = targets_layout(want, len(tells), channels)
    got_csr = audio.targets(plan, tells, bins, mfma=False)
    got = audio.targets(plan, tells, bins, mfma=True)
    assert np.array_equal(got_csr.astype(np.float64), want), np.argwhere(got_csr != want)[:4].tolist()
    assert np.array_equal(got, got_csr), np.argwhere(got != got_csr)[:4].tolist()
    N.check(gpu.lib.sfx_stft_plan_destroy(plan))
    N.check(gpu.lib.sfx_audio_destroy(audio.handle))


def test_mfma_scratch_grows_and_is_reused(gpu):
    """sfx_spectrogram_targets on one plan with mfma = 1 for 1, then 40, then 3 frames: the k-split scratch and the plan's buffers grow, then
    serve a smaller call whose column stride differs — each result is a fresh plan's"""
    fft_n, bins, channels = 6, 33, 2
    n = 1 << fft_n
    rng = np.random.default_rng(7)
    pcm = (0.4*rng.standard_normal((R.stream_total(n), channels))).astype(np.float32)
    csr = R.csr_matrix("a", bins, n//2 + 1)
    audio = Audio(gpu, pcm)
    kept = audio.plan(fft_n, 0, *csr, bins)
    for frames in (1, 40, 3):
        tells = np.linspace(n//2, len(pcm) + n//2, frames + 2).astype(np.int64)[1:-1]
        fresh = audio.plan(fft_n, 0, *csr, bins)
        want = audio.targets(fresh, tells, bins, mfma=True)
        N.check(gpu.lib.sfx_stft_plan_destroy(fresh))
        got = audio.targets(kept, tells, bins, mfma=True)
        assert want.any() and np.array_equal(got, want), frames
        assert np.array_equal(audio.targets(kept, tells, bins, mfma=False), np.stack([O.csr_dot(*csr, p) for p in audio.power(kept, tells, fft_n)]))
    N.check(gpu.lib.sfx_stft_plan_destroy(kept))
    N.check(gpu.lib.sfx_audio_destroy(audio.handle))
