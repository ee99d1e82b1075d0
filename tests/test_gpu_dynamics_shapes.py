"""
The dynamics scans (k_dynamics_scan, k_dynamics_scan_f64) at every instance the launcher has, at the limits between them, with every kind
of system and clock of tests/dynamics_cases.py, with targets that are not finite, with many float64 systems, and through the tape with
SNAPSHOT, the keeper thread, the loudness systems and the uniforms. Every comparison is exact: the kernels restate the reference's float
operations one by one, so the oracle's bits (and the host DynamicNumber's, for the snapshot) are the expected value.

Which instance a value count takes (launch_dynamics_scan_as, csrc/capi_audio.hip): n <= 256 <64, 4, keeper wave>, <= 2048 <1024, 2>,
<= 4096 <1024, 4>, <= 8192 <1024, 8>, above <1024, 16>; sfx_dynamics_scan takes the forms without SNAPSHOT, a tape with sfx_tape_snapshot
the forms with it.
"""
import ctypes as C

import numpy as np
import pytest

from shaderflow_amd import _native as N
from tests import dynamics_cases as D
from tests.test_gpu_audio import Audio, _coeff_table, gpu, trivial_csr  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def scan(gpu, targets, coeff, state, calls, precision=D.PRECISION):
    """sfx_dynamics_scan over consecutive calls of `calls` frames each, the state array carried from call to call"""
    n = targets.shape[1]
    got = np.full_like(targets, -7.0)
    first = 0
    for count in calls:
        chunk, table = np.ascontiguousarray(targets[first:first + count]), np.ascontiguousarray(coeff[first:first + count])
        N.check(gpu.lib.sfx_dynamics_scan(gpu.ctx.handle, count, n, N.as_ptr(chunk, C.c_float), C.cast(table.ctypes.data, C.POINTER(N.DynCoeffF32)),
                                          np.float32(precision), N.as_ptr(state, C.c_float), N.as_ptr(got[first:], C.c_float)))
        first += count
    assert first == len(targets)
    return got


def first_difference(got, want):
    where = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    if not len(where):
        return None
    at = tuple(int(i) for i in where[0])
    return f"{len(where)} values differ, first at (frame, index) {at}: expected {want[at]!r}, device {got[at]!r}"


@pytest.mark.parametrize("n,params", D.SCAN_CASES)
def test_scan_at_every_instance_limit_and_parameter_set(gpu, n, params):
    """Four calls of 1, 1, 58 and 100 frames: a call whose only frame has dt = 0, a one-frame call (nothing to prefetch), two hand-overs;
    every frame and the returned state bit for bit the oracle's"""
    targets, dts, coeff, oracle = D.scan_reference(n, params)
    assert np.array_equal(coeff, _coeff_table(*params, dts, np.float32))
    state = np.zeros(3*n, np.float32)
    got = scan(gpu, targets, coeff, state, D.SCAN_CALLS)
    assert np.array_equal(got, oracle.values), first_difference(got, oracle.values)
    assert np.array_equal(state[:n], oracle.values[-1])
    assert np.array_equal(state[n:2*n], oracle.derivatives[-1])
    assert np.array_equal(state[2*n:], oracle.previous)


@pytest.mark.parametrize("n,kind", D.NONFINITE_CASES)
def test_scan_steps_where_the_early_outs_maximum_is_nan(gpu, n, kind):
    """np.abs(target - value).max() is NaN as soon as one difference is: the comparison with the precision is false and the whole array
    steps (dynamics.py:222-225), where every finite value has long converged. A maximum that drops NaN operands freezes the array instead.

    The kernel before this test (fmaxf in the lane loop, across the wave and over the waves' maxima) froze there; the first wrong values are
    finite ones, whose low bits a step of a converged system still moves — (frame, index): expected, device
      n = 300  a (80, 4): 0.9535631, 0.95356303     b (82, 4): 0.11816113, 0.118161134    c (80, 0): 1.4088805, 1.4088804
      n = 200  a (80, 0): 2.98238, 2.9823797        b (82, 1): 0.43975228, 0.4397523      c (80, 0): 0.5444229, 0.544423
    (b: the -inf target makes the maximum infinite on frames 80 and 81, so the old kernel stepped there too; from frame 82 the difference
    -inf - -inf is NaN)."""
    targets, dts, coeff = D.nonfinite_case(n, kind)
    oracle = D.oracle_f32(D.NONFINITE_PARAMS, targets, dts)
    assert np.isnan(oracle.values[80:]).any()
    state = np.zeros(3*n, np.float32)
    got = scan(gpu, targets, coeff, state, D.NONFINITE_CALLS)
    assert np.array_equal(got, oracle.values, equal_nan=True), first_difference(got, oracle.values)
    infinite = np.isinf(oracle.values)
    assert np.array_equal(np.isinf(got), infinite) and np.array_equal(np.signbit(got[infinite]), np.signbit(oracle.values[infinite]))
    for block, want in ((state[:n], oracle.values[-1]), (state[n:2*n], oracle.derivatives[-1]), (state[2*n:], oracle.previous)):
        assert np.array_equal(block, want, equal_nan=True), first_difference(block, want)
        assert np.array_equal(np.signbit(block[np.isinf(want)]), np.signbit(want[np.isinf(want)]))


@pytest.mark.parametrize("n,where", D.EDGE_CASES)
def test_scan_early_out_at_the_precision_itself(gpu, n, where):
    """One value just below the precision, every other at its target: frozen, `previous` included (the state after the first call).
    The same value at the precision: the array steps (the second call). The device's maximum has to be exact to the last bit for both."""
    targets, dts, coeff = D.precision_edge_case(n, where)
    host = D.host_f32(D.EDGE_PARAMS, targets, dts)
    oracle = D.oracle_f32(D.EDGE_PARAMS, targets, dts)
    state = np.zeros(3*n, np.float32)
    got = scan(gpu, targets[:D.EDGE_CALLS[0]], coeff[:D.EDGE_CALLS[0]], state, D.EDGE_CALLS[:1])
    assert not got.any() and not state.any(), first_difference(state, np.zeros_like(state))
    rest = scan(gpu, targets[D.EDGE_CALLS[0]:], coeff[D.EDGE_CALLS[0]:], state, D.EDGE_CALLS[1:])
    assert np.array_equal(rest, oracle.values[D.EDGE_CALLS[0]:]), first_difference(rest, oracle.values[D.EDGE_CALLS[0]:])
    assert rest[-1, where] != 0
    for block, want in ((state[:n], host.values[-1]), (state[n:2*n], host.derivatives[-1]), (state[2*n:], host.previous[-1])):
        assert np.array_equal(block, want), first_difference(block, want)


@pytest.mark.parametrize("integrate", [0, 1])
@pytest.mark.parametrize("nsystems,with_nan", [(n, False) for n in D.F64_SYSTEMS] + [(9, True)])
def test_scalar_scan_of_many_systems(gpu, nsystems, with_nan, integrate):
    """Coefficients are [system][frame], targets and outputs [frame][system]: with parameters, tracks and start values of its own per system
    a transposed index shows. 65 and 130 systems reach the second and third block. Two calls."""
    params, starts, targets, dts, coeff = D.scalar_case(nsystems, with_nan)
    count = len(params)
    want = np.stack([D.oracle_f64(params[k], starts[k], targets[:, k], dts, integrate) for k in range(count)], axis=1)   # (frames, systems, 4)
    state = np.ascontiguousarray(np.stack([starts, np.zeros(count), starts, np.zeros(count)], axis=1))                  # value, derivative, previous, integral
    got = np.full((D.FRAMES, count, 3), -7.0)
    first = 0
    for frames in D.F64_CALLS:
        chunk = np.ascontiguousarray(targets[first:first + frames])
        table = np.ascontiguousarray(coeff[:, first:first + frames])
        out = np.full((frames, count, 3), -7.0)
        N.check(gpu.lib.sfx_dynamics_scan_f64(gpu.ctx.handle, frames, count, N.as_ptr(chunk, C.c_double), C.cast(table.ctypes.data, C.POINTER(N.DynCoeffF64)),
                                              D.PRECISION, integrate, N.as_ptr(state, C.c_double), N.as_ptr(out, C.c_double)))
        got[first:first + frames] = out
        first += frames
    assert first == D.FRAMES
    for k in range(count):
        nan = with_nan and k == count - 1
        for field, name in enumerate(("value", "integral", "derivative")):
            assert np.array_equal(got[:, k, field], want[:, k, field], equal_nan=nan), (k, params[k], name, first_difference(got[:, k, field], want[:, k, field]))
        final = want[-1, k, [0, 2, 3, 1]]                             # the state's order: value, derivative, previous, integral
        assert np.array_equal(state[k], final, equal_nan=nan), (k, params[k], state[k], final)
    if with_nan:
        # (the NaN reaches the derivative on frame 80 and the value, which moves by the derivative of the frame before, on frame 81)
        assert np.isnan(got[80:, -1, 2]).all() and np.isnan(got[81:, -1, 0]).all() and np.isfinite(got[:80, -1]).all() and np.isfinite(got[:, :-1]).all()


# ---- the tape path -----------------------------------------------------------------------------------------------
FPS, RATE = 60, 44100
TAPE_FRAMES, TAPE_BATCHES = 100, (37, 63)
SPECTRUM, VOLUME, STD = (8, 1, 0), (2, 1, 0), (10, 1, 0)
# (stereo bins, fft_n, snapshot): n = 258 and 2048 take <1024, 2>, 2050 <1024, 4>, 4098 <1024, 8>, 16384 <1024, 16>
TAPE_SHAPES = [(bins, fft_n, snapshot) for bins, fft_n in ((129, 11), (1024, 11), (1025, 11), (2049, 12)) for snapshot in (False, True)] + [(8192, 14, True)]


def tape_clip(frames):
    """0.3 s of noise, digital silence, noise again from the 96th frame's samples on. Silence gives targets and loudness of exactly 0: the
    bins and the two float64 systems converge, freeze and move again. The noise is quiet (sigma = 1e-3) so that the 2 Hz volume system gets
    within its precision of 1e-6 during the silence these frames have room for."""
    rng = np.random.default_rng(31)
    pcm = np.zeros(((frames + 1)*RATE//FPS, 2), np.float32)
    head, resume = int(0.3*RATE), (frames - 5)*RATE//FPS
    pcm[:head] = (1e-3*rng.standard_normal((head, 2))).astype(np.float32)
    pcm[resume:] = (1e-3*rng.standard_normal((len(pcm) - resume, 2))).astype(np.float32)
    return pcm


def frozen_then_moving(trajectory, dts, least):
    """At least `least` frames equal to the frame before them (dt != 0), and a later frame that differs"""
    frozen = D.frozen_frames(trajectory, dts, 2, len(trajectory))
    return len(frozen) >= least and not np.array_equal(trajectory[-1], trajectory[frozen[-1]])


@pytest.mark.parametrize("bins,fft_n,snapshot", TAPE_SHAPES)
def test_tape_scan_with_keeper_loudness_uniforms_and_snapshot(gpu, bins, fft_n, snapshot):
    """sfx_tape_create / sfx_tape_snapshot / sfx_tape_build / sfx_tape_read over a trivial filterbank of `bins` rows: the 1024-thread
    instances with thread 0 as the keeper of the float64 loudness systems and the uniforms, without and with the per-frame state snapshot.
    Expected values from the device's own analysis: O.DynF32 fed TAPE_TARGETS, O.DynF64 fed TAPE_LOUDNESS.
    (The 8192-bin shape runs the 100 frames of the others: its transform of 16 384 samples alone spans 22 frames, and the trajectory has to
    converge, stay frozen for 20 frames and move again.)"""
    frames, n = TAPE_FRAMES, 2*bins
    audio = Audio(gpu, tape_clip(frames), RATE)
    plan = audio.plan(fft_n, 0, *trivial_csr(bins), bins)
    desc = N.TapeDesc(points=0, chunk_size=1, reducer=0, volume_window=RATE//10, use_mfma=0, volume_integrate=1, std_integrate=0, precision=D.PRECISION)
    tape = N.Handle()
    N.check(gpu.lib.sfx_tape_create(plan, audio.handle, C.byref(desc), max(TAPE_BATCHES), C.byref(tape)))
    if snapshot:
        N.check(gpu.lib.sfx_tape_snapshot(tape, 1))

    dts = np.full(frames, 1/FPS); dts[0] = 0.0
    spec_c, vol_c, std_c = _coeff_table(*SPECTRUM, dts, np.float32), _coeff_table(*VOLUME, dts, np.float64), _coeff_table(*STD, dts, np.float64)
    clock = np.zeros(frames, dtype=[("iTime", "f4"), ("iTau", "f4"), ("iSpectrogramOffset", "f4"), ("iFrame", "i4")])
    clock["iTime"] = np.arange(frames)/FPS; clock["iTau"] = np.arange(frames)/frames; clock["iSpectrogramOffset"] = np.arange(frames) % 7; clock["iFrame"] = np.arange(frames)
    tells = (np.arange(frames, dtype=np.int64) + 1)*(RATE//FPS)

    sections = {N.TAPE_SPECTROGRAM: ((n,), np.float32), N.TAPE_TARGETS: ((n,), np.float32), N.TAPE_LOUDNESS: ((2,), np.float32), N.TAPE_UNIFORMS: ((8,), np.float32)}
    read = {what: [] for what in sections}
    state64, state32 = [], []
    first = 0
    for count in TAPE_BATCHES:
        s = slice(first, first + count)
        args = [np.ascontiguousarray(a[s]) for a in (tells, clock, spec_c, vol_c, std_c)]
        N.check(gpu.lib.sfx_tape_build(tape, count, N.as_ptr(args[0], C.c_int64), C.cast(args[1].ctypes.data, C.POINTER(N.FrameClock)),
                                       C.cast(args[2].ctypes.data, C.POINTER(N.DynCoeffF32)), C.cast(args[3].ctypes.data, C.POINTER(N.DynCoeffF64)),
                                       C.cast(args[4].ctypes.data, C.POINTER(N.DynCoeffF64))))
        for what, (shape, dtype) in sections.items():
            out = np.full((count,) + shape, -7.0, dtype)
            N.check(gpu.lib.sfx_tape_read(tape, what, 0, count, out.ctypes.data, out.nbytes))
            read[what].append(out)
        if snapshot:
            raw = np.zeros(count*(96 + 24*n), np.uint8)
            N.check(gpu.lib.sfx_tape_read(tape, N.TAPE_STATE, 0, count, raw.ctypes.data, raw.nbytes))
            state64.append(raw[:count*96].view(np.float64).reshape(count, 2, 6).copy())
            state32.append(raw[count*96:].view(np.float32).reshape(count, 6, n).copy())
        first += count
    assert first == frames
    N.check(gpu.lib.sfx_tape_destroy(tape))
    columns, targets, loudness, uniforms = (np.concatenate(read[what]) for what in (N.TAPE_SPECTROGRAM, N.TAPE_TARGETS, N.TAPE_LOUDNESS, N.TAPE_UNIFORMS))

    # the analysis gave what the clip promises: exact zeros in the silence, sound before and after
    silent = [k for k in range(frames) if not targets[k].any() and not loudness[k].any()]
    assert len(silent) >= 40 and targets[:10].any(axis=1).all() and targets[-1].any() and loudness[-1].all()

    # the bins: the oracle on the device's own targets, and a trajectory that freezes and moves again
    want = D.oracle_f32(SPECTRUM, targets, dts)
    assert frozen_then_moving(want.values, dts, 20), "the clip's silence is too short for the bins to freeze"
    assert np.array_equal(columns, want.values), first_difference(columns, want.values)

    # the loudness systems: value, integral, derivative, previous of every frame; the uniforms carry them rounded to float32
    volume = D.oracle_f64(VOLUME, 0.0, loudness[:, 0], dts, integrate=1)
    std = D.oracle_f64(STD, 0.0, loudness[:, 1], dts, integrate=0)
    assert frozen_then_moving(std[:, 0], dts, 20), "the clip's silence is too short for the std system to freeze"
    # (at 2 Hz the volume needs some 57 frames of silence to come within 1e-6: it freezes for the last ones, its integral running on)
    assert frozen_then_moving(volume[:, 0], dts, 8), "the clip's silence is too short for the volume system to freeze"
    assert np.array_equal(uniforms[:, 2], volume[:, 0].astype(np.float32)), first_difference(uniforms[:, 2], volume[:, 0].astype(np.float32))
    assert np.array_equal(uniforms[:, 3], volume[:, 1].astype(np.float32)) and volume[-1, 1] != 0
    assert np.array_equal(uniforms[:, 4], std[:, 0].astype(np.float32)), first_difference(uniforms[:, 4], std[:, 0].astype(np.float32))
    assert np.array_equal(uniforms[:, 0], clock["iTime"]) and np.array_equal(uniforms[:, 1], clock["iTau"])
    assert np.array_equal(uniforms[:, 5], clock["iSpectrogramOffset"]) and np.array_equal(uniforms[:, 6].view(np.int32), clock["iFrame"])
    assert not uniforms[:, 7].view(np.int32).any()

    if snapshot:
        # value, target, previous, derivative, acceleration, integral after every frame's update(): what the host objects hold. A frozen
        # frame (and a dt = 0 frame) takes the new target and leaves `previous` — the target of the last step — and the rest alone.
        state64, state32 = np.concatenate(state64), np.concatenate(state32)
        host = D.host_f32(SPECTRUM, targets, dts)
        assert np.array_equal(host.values, want.values)
        for field, name in enumerate(("values", "targets", "previous", "derivatives", "accelerations")):
            assert np.array_equal(state32[:, field], getattr(host, name)), (name, first_difference(state32[:, field], getattr(host, name)))
        assert not state32[:, 5].any()                               # the bins never integrate
        for system, (params, integrate, oracle) in enumerate(((VOLUME, 1, volume), (STD, 0, std))):
            mirror = D.host_f64(params, 0.0, loudness[:, system], dts, integrate, float32_targets=True)
            assert np.array_equal(mirror[:, 0], oracle[:, 0]) and np.array_equal(mirror[:, 5], oracle[:, 1])
            for field, name in enumerate(("value", "target", "previous", "derivative", "acceleration", "integral")):
                assert np.array_equal(state64[:, system, field], mirror[:, field]), (system, name, first_difference(state64[:, system, field], mirror[:, field]))
