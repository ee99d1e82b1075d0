"""
Plain float64 references of the STFT and filterbank kernels (csrc/audio_kernels.hpp: k_stft_power, k_dft_power, k_filterbank_csr,
k_filterbank_mfma + k_filterbank_reduce), the bounds they are held to, and the shapes and signals both the CPU and the GPU tests use.
No device code: numpy's rfft on the oracle's float64 window table. tests/test_host_audio_ref.py holds these references and bounds to the
oracle's own transform and CSR product; tests/test_gpu_audio_shapes.py holds the kernels to them.

The STFT bound, per bin, on |got - want64| (`stft_bound`): one float32 ulp of the rounded value — the kernels transform in float64 and
round once — plus STFT_K*sqrt(want64*peak) for the float64 transform's own error (an error e on a bin of magnitude |X| moves the power
by 2|X|e, and e scales with the frame's largest bin), plus the smallest float32 subnormal. STFT_K is not taken from any device: it is
the disagreement of the two independent float64 transforms that exist on the CPU, numpy's pocketfft and the oracle's radix-2
(sfo_fft_power), measured over the signals of `signals()`, the three windows and fft_n 4 to 14 at the five tells of `tells()`:
    the oracle's float32 power lay at most 2.6e-16*sqrt(want64*peak) beyond one ulp of numpy's float64 power (2.5e-16 at fft_n 13,
    2.3e-16 at 10 and 12, 2.2e-16 at 14, 0.8e-16 at 11; above zero on 0.03 % of the bins at fft_n 10 to 14, the floor of the sine-plus-
    noise spectra, and nowhere below 10; test_host_audio_ref.py measures the figure again on every run),
times a margin of 16, because the device's butterfly order (a packed half-size transform and a split) is a third one:
    STFT_K = 16 * 2.6e-16 = 4.16e-15.
Amplitudes take the same form on the magnitude: one ulp + STFT_K*peak amplitude. Complex float64 pairs have no float32 rounding: STFT_K*
sqrt(peak power) on |got - want| alone. (A measurement over other signals of the same kinds gave 1.1e-16; the larger figure is kept.)
stft_bound is first order in the transform's error; `second_order` is the term it leaves out, (STFT_K/2)**2*peak, which the GPU test
adds for power: it is all that is left at a bin where the true spectrum is exactly zero.

The filterbank bound is derived, not measured: a row of n stored entries is summed by the MFMA path with at most n float32 roundings
in its fma chains (products are exact inside an fma; a column stored twice costs one rounding when the dense matrix adds the two
weights, and one entry less in the chain) and FILTERBANK_SPLITS roundings when the partial sums are added, so in ANY order
|got - want64| <= gamma(n + FILTERBANK_SPLITS)*S with gamma(m) = m*u/(1 - m*u), u = 2**-24 and S = sum |a_k*p_k| (Higham, Accuracy and
Stability of Numerical Algorithms, §3.1 and §4.2). The CSR kernel claims more: the bits of `csr_loop_f32`, scipy's order.
"""
from __future__ import annotations

import numpy as np

from oracle import binding as O

STFT_K_MEASURED = 2.6e-16
STFT_K_MARGIN = 16
STFT_K = STFT_K_MARGIN*STFT_K_MEASURED
TINY = float(np.finfo(np.float32).smallest_subnormal)
FILTERBANK_SPLITS = 8                                               # csrc/audio_kernels.hpp
U = 2.0**-24

FFT_NS = tuple(range(4, 15))
WINDOWS = (0, 1, 2)                                                 # hanning, hann_poisson, none (include/shaderflow_hip.h)
SIGNALS = ("sine_noise", "sine_dc", "impulses", "silence")
RESAMPLED = ((4, 24), (4, 48), (6, 96), (8, 384), (8, 768), (9, 1536))      # (fft_n, fft_size): none a power of two, so k_dft_power


def stream_total(n: int) -> int:
    return 3*n + 7


def tells(n: int) -> np.ndarray:
    """The ring after 1 sample (all zeros in front), half a window, one window and a sample, the whole stream, and half a window past its
    end (zeros behind)"""
    total = stream_total(n)
    return np.array([1, n//2, n + 1, total, total + n//2], np.int64)


def signals(channels: int, n: int) -> dict[str, np.ndarray]:
    """Planar (channels, 3n + 7) float32 streams: a loud sine off the bin centres plus noise at 1e-7 of it (the spectrum's floor lies
    fourteen decades under its peak), a sine on a DC offset, one impulse per channel at its own offset and amplitude, silence"""
    total = stream_total(n)
    rng = np.random.default_rng(100*n + channels)
    t = np.arange(total, dtype=np.float64)
    out = {name: np.zeros((channels, total)) for name in SIGNALS}
    for c in range(channels):
        cycles = (n/8 + 0.37*(c + 1))/n
        out["sine_noise"][c] = 0.9*np.sin(2*np.pi*cycles*t + 0.3*c) + 0.9e-7*rng.standard_normal(total)
        out["sine_dc"][c] = 0.3*np.sin(2*np.pi*(cycles/2)*t + 1.1*c) + (0.5, -0.25, 0.125)[c % 3]
        for k, start in enumerate((n//3 + 2*c + 1, n + 3 + c, 3*n + c)):            # the last one lies in both of the last two frames
            out["impulses"][c, start] = (1.0, -0.75, 0.3)[c % 3]*(1 + k)
    return {name: np.ascontiguousarray(s, np.float32) for name, s in out.items()}


def stream_frame(pcm: np.ndarray, tell: int, n: int) -> np.ndarray:
    """The samples tell - n - 1 … tell - 2 of the planar stream (audio/module.py:137-138 leaves the newest sample out), zeros outside it"""
    pcm = np.asarray(pcm)
    total = pcm.shape[1]
    idx = np.arange(tell - n - 1, tell - 1)
    inside = (idx >= 0) & (idx < total)
    frame = np.zeros((pcm.shape[0], n), pcm.dtype)
    frame[:, inside] = pcm[:, idx[inside]]
    return frame


def _magnitude(spectrum: np.ndarray, what: str) -> np.ndarray:
    if what == "power":
        return spectrum.real**2 + spectrum.imag**2
    if what == "amplitude":
        return np.abs(spectrum)
    assert what == "complex", what
    return spectrum


def stft_ref(pcm: np.ndarray, tell: int, fft_n: int, window: int, what: str = "power") -> np.ndarray:
    """float64 (channels, N/2 + 1): np.fft.rfft of the float64 window times the frame; `what` = power, amplitude or complex"""
    n = 1 << fft_n
    frame = stream_frame(pcm, tell, n).astype(np.float64)
    return _magnitude(np.fft.rfft(O.window(window, n)*frame, axis=-1), what)


def resampled_input(pcm: np.ndarray, tell: int, fft_n: int, ratio: float, fft_size: int) -> np.ndarray:
    """The transform's inputs under `sample_rateio` = ratio, as stft_input of the kernel applies the taps: the frame of 2**fft_n samples
    interpolated in float64 at linear_resample_taps' positions and rounded to float32 (the converter writes float32). (channels, fft_size)"""
    from shaderflow_amd.audio.spectrogram import linear_resample_taps
    a, b, w = linear_resample_taps(1 << fft_n, ratio, fft_size)
    assert len(a) == fft_size, (len(a), fft_size)
    frame = stream_frame(pcm, tell, 1 << fft_n).astype(np.float64)
    return (frame[:, a] + w*(frame[:, b] - frame[:, a])).astype(np.float32)


def resampled_ref(pcm: np.ndarray, tell: int, fft_n: int, fft_size: int, window: int, what: str = "power") -> np.ndarray:
    """The same rfft over the resampled inputs and the window of fft_size samples"""
    data = resampled_input(pcm, tell, fft_n, fft_size/(1 << fft_n), fft_size).astype(np.float64)
    return _magnitude(np.fft.rfft(O.window(window, fft_size)*data, axis=-1), what)


def stft_bound(want64: np.ndarray) -> np.ndarray:
    """Allowed |got - want64| of float32 power spectra (…, bins); the peak is each spectrum's own"""
    peak = want64.max(axis=-1, keepdims=True)
    return np.spacing(want64.astype(np.float32)).astype(np.float64) + STFT_K*np.sqrt(want64*peak) + TINY


def second_order(want64: np.ndarray) -> np.ndarray:
    """The term stft_bound leaves out. A transform error e on a bin X moves the power by 2 Re(conj(X) e) + |e|**2; STFT_K*sqrt(want*peak)
    is the first term with |e| <= STFT_K/2*sqrt(peak), so the second is (STFT_K/2)**2 * peak — thirty decades under the peak, and all
    that is left where the true spectrum is exactly zero: a linearly resampled impulse is a triangle, whose spectrum under the window
    `none` vanishes at N/3 (numpy returns 0.0 there, any plain sum the square of its rounding error, about 1e-32 of the peak)."""
    return (STFT_K/2)**2*want64.max(axis=-1, keepdims=True)


def amplitude_bound(want64: np.ndarray) -> np.ndarray:
    peak = want64.max(axis=-1, keepdims=True)
    return np.spacing(want64.astype(np.float32)).astype(np.float64) + STFT_K*peak + TINY


def complex_bound(want: np.ndarray) -> np.ndarray:
    """Allowed |got - want| of the float64 complex spectrum: the transform's error alone"""
    return STFT_K*np.abs(want).max(axis=-1, keepdims=True)


def stft_excess(got: np.ndarray, want64: np.ndarray) -> float:
    """What a float32 power spectrum lies beyond one ulp (and the subnormal) of want64, in units of sqrt(want64*peak): the measure of STFT_K"""
    peak = want64.max(axis=-1, keepdims=True)
    beyond = np.abs(got.astype(np.float64) - want64) - np.spacing(want64.astype(np.float32)).astype(np.float64) - TINY
    scale = np.sqrt(want64*peak)
    return float(np.max(np.where(scale > 0, beyond/np.where(scale > 0, scale, 1.0), 0.0), initial=0.0))


def worst_ratio(got: np.ndarray, want: np.ndarray, bound: np.ndarray) -> float:
    """max |got - want| / bound over the values that differ at all: at most 1 when the bound holds"""
    error = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(error > 0, error/bound, 0.0)
    return float(ratio.max(initial=0.0))


def filterbank_ref(indptr, indices, data, power: np.ndarray):
    """power: (columns, fft_bins) float32. Returns the float64 product (bins, columns), S = sum |a_k*p_k| of the same shape, and the
    rows' entry counts n (bins,). Entries are taken as stored: a column named twice counts twice."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    a, p = np.asarray(data, np.float32).astype(np.float64), np.asarray(power, np.float32).astype(np.float64)
    bins = len(indptr) - 1
    want, size = np.zeros((bins, p.shape[0])), np.zeros((bins, p.shape[0]))
    for r in range(bins):
        j = slice(indptr[r], indptr[r + 1])
        terms = a[j]*p[:, indices[j]]                                # (columns, n)
        want[r], size[r] = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    return want, size, np.diff(indptr)


def gamma(m):
    m = np.asarray(m, np.float64)
    return m*U/(1.0 - m*U)


def filterbank_bound(size: np.ndarray, n: np.ndarray) -> np.ndarray:
    return gamma(n + FILTERBANK_SPLITS)[:, None]*size


def csr_loop_f32(indptr, indices, data, power: np.ndarray) -> np.ndarray:
    """scipy's csr_matvecs in numpy float32: a row's entries in the order they are stored, a multiply, then an add. (bins, columns)"""
    a, p = np.asarray(data, np.float32), np.asarray(power, np.float32)
    bins = len(indptr) - 1
    out = np.zeros((bins, p.shape[0]), np.float32)
    for r in range(bins):
        acc = np.zeros(p.shape[0], np.float32)
        for j in range(int(indptr[r]), int(indptr[r + 1])):
            prod = a[j]*p[:, int(indices[j])]
            acc = acc + prod
        out[r] = acc
    return out


# ---- CSR matrices of the tests' own --------------------------------------------------------------------------------------------------
# kinds: a banded triangles of 3-4 entries (the reference's shape), b a whole 32-row tile and single rows elsewhere without entries,
# c one fully dense row, d rows stored out of column order, e weights of both signs, f columns named more than once, g no entries at all

KINDS = "abcdefg"


def _banded_rows(bins: int, fft_bins: int, rng) -> list[tuple[np.ndarray, np.ndarray]]:
    rows = []
    for r in range(bins):
        centre = int(round((r + 1)*(fft_bins - 1)/bins))
        width = int(rng.integers(3, 5))
        first = min(max(centre - 1, 0), fft_bins - width)              # the last row ends on the last fft bin
        cols = np.arange(first, first + width)
        rows.append((cols, rng.uniform(0.05, 1.0, width)))
    return rows


def csr_matrix(kind: str, bins: int, fft_bins: int, seed: int = 0, exact: bool = False):
    """(indptr, indices, data) int32 / int32 / float32. `exact`: weights are integers in -8 … 8 over 1, 2, 4 or 8 — with powers that are
    powers of two, every partial sum of a row is a float32 in any order"""
    rng = np.random.default_rng(1000*seed + 10*bins + fft_bins + ord(kind))
    rows = _banded_rows(bins, fft_bins, rng)
    if kind == "b":
        for r in range(bins):
            if 32 <= r < 64 or r in (5, 17):
                rows[r] = (np.zeros(0, np.int64), np.zeros(0))
    if kind == "c":
        rows[bins//2] = (np.arange(fft_bins), rng.uniform(0.05, 1.0, fft_bins))
    if kind == "d":
        for r in range(bins):
            count = min(int(rng.integers(4, 7)), fft_bins)
            first = min(rows[r][0][0], fft_bins - count)
            rows[r] = (rng.permutation(np.arange(first, first + count)), rng.uniform(0.05, 1.0, count))
    if kind == "e":
        rows = [(cols, weights*rng.choice([-1.0, 1.0], len(cols))) for cols, weights in rows]
    if kind == "f":
        for r in range(bins):
            cols = rows[r][0]
            cols = np.concatenate([cols, cols[[0, 0, 1]] if r % 2 else cols[[1]]])       # a column three times and another twice, or one twice
            rows[r] = (rng.permutation(cols), rng.uniform(0.05, 1.0, len(cols)))
    if kind == "g":
        rows = [(np.zeros(0, np.int64), np.zeros(0))]*bins
    if exact:
        rows = [(cols, rng.integers(-8, 9, len(cols))/2.0**rng.integers(0, 4, len(cols))) for cols, _ in rows]
    indptr = np.concatenate([[0], np.cumsum([len(cols) for cols, _ in rows])]).astype(np.int32)
    indices = np.concatenate([cols for cols, _ in rows]).astype(np.int32)
    data = np.concatenate([weights for _, weights in rows]).astype(np.float32)
    return indptr, indices, data


def exact_matrix(bins: int, fft_bins: int, seed: int = 0):
    """Every kind of row in one matrix with exact weights: banded, unsorted and repeated columns in turn, the last row fully dense, row 3
    without entries"""
    parts = {kind: csr_matrix(kind, bins, fft_bins, seed, exact=True) for kind in "acdf"}
    rows = []
    for r in range(bins):
        indptr, indices, data = parts["c" if r == bins - 1 else "adf"[r % 3]]
        source = bins//2 if r == bins - 1 else r                      # (kind c keeps its dense row in the middle)
        rows.append((indices[indptr[source]:indptr[source + 1]], data[indptr[source]:indptr[source + 1]]) if r != 3 else (indices[:0], data[:0]))
    indptr = np.concatenate([[0], np.cumsum([len(cols) for cols, _ in rows])]).astype(np.int32)
    return indptr, np.concatenate([cols for cols, _ in rows]).astype(np.int32), np.concatenate([weights for _, weights in rows]).astype(np.float32)


EXACT_AMPLITUDES = (1.0, 2.0, -0.5)                                   # powers 1, 4, 0.25 in every bin under the window `none`


def exact_stream(channels: int, n: int) -> tuple[np.ndarray, np.ndarray]:
    """(planar stream of 2n samples with one impulse per channel, the tells whose frame holds every channel's impulse)"""
    pcm = np.zeros((channels, 2*n), np.float32)
    for c in range(channels):
        pcm[c, n - 3 - c] = EXACT_AMPLITUDES[c]
    return pcm, np.arange(n - 1, 2*n - 3, dtype=np.int64)            # impulse p in [tell - n - 1, tell - 2] for p = n - 5 … n - 3
