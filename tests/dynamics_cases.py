"""
Inputs and references of the dynamics-scan tests (test_host_dynamics_cases.py on the CPU, test_gpu_dynamics_shapes.py on the device):
DynamicNumber.next (dynamics.py:197-250) over parameter sets that take both coefficient branches, ring, creep and use the velocity term,
a clock with dt = 0 frames and a variable dt, targets that converge, freeze and move again, and targets that are not finite. No GPU here.

Two references, stepped frame by frame: the oracle (O.DynF32 / O.DynF64, the expected value) and the host class
shaderflow_amd.dynamics.DynamicNumber, which also holds `previous` and `acceleration` (what the tape's state snapshot carries).
"""
from __future__ import annotations

from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from oracle import binding as O
from shaderflow_amd.dynamics import DynamicNumber, dynamics_coefficients

# (frequency, zeta, response). FREEZING sets converge within the hold and take the early-out (dynamics.py:222-225); MOVING sets ring or
# creep for the whole run and never reach it.
FREEZING = [(4, 1, 0), (8, 1, 0), (6, 0.5, 0), (40, 1, 0), (40, 0.4, 1), (40, 3, 0), (12, 1.5, -2)]
MOVING = [(3, 0.3, 2), (2, 2.5, -1)]
PARAMS = FREEZING + MOVING
# the coefficient branches (dynamics_coefficients) each set takes over the clock's non-zero dts
BRANCHES = {(4, 1, 0): {0}, (40, 1, 0): {1}, (40, 0.4, 1): {1}, (2, 2.5, -1): {0}}          # every other set: both

PRECISION = 1e-6
FRAMES = 160
HOLD = (10, 125)                     # rows 10 to 124 of the targets equal row 10
# every limit of the launcher's instances (1, 64 | 65, 256 | 257, 2048 | 4096 | 8192) and their neighbours
SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 4096, 8192)
EVERY_SET_AT = (65, 257, 2048)
SCAN_CASES = [(n, (8, 1, 0)) for n in SIZES] + [(n, p) for n in EVERY_SET_AT for p in PARAMS if p != (8, 1, 0)]
SCAN_CALLS = (1, 1, 58, 100)         # a call whose only frame has dt = 0, a one-frame call, two hand-overs


def coeff_table(freq, zeta, resp, dts, dtype):
    """As tests/test_gpu_audio.py `_coeff_table`: the python scalars (dt, k1, k2, k3) of every frame, rounded to `dtype` the way numpy
    rounds them for an array of that dtype; a dt = 0 frame is a row of zeros"""
    wide = np.zeros((len(dts), 4), np.float64)
    for k, dt in enumerate(dts):
        dt = abs(float(dt))
        if dt:
            k1, k2, k3, _ = dynamics_coefficients(freq, zeta, resp, dt)
            wide[k] = (dt, k1, k2, k3)
    return np.ascontiguousarray(wide.astype(dtype))


def clock(frames=FRAMES):
    """dt per frame: 1/60, dt = 0 on frame 0 and frame 130, fifteen frames of a variable dt"""
    dts = np.full(frames, 1/60)
    dts[0] = 0.0
    if frames > 150:
        dts[130] = 0.0
        # (seed 2: every drawn dt lies between 1/(tau*40) and 1/(tau*4), so (4,1,0) stays in branch 0 and (40,1,0) in branch 1, and some
        # lie on either side of 1/60's branch for the sets in between — test_host_dynamics_cases.py asserts the coverage)
        dts[135:150] = np.random.default_rng(2).uniform(0.002, 0.04, 15)
    return dts


def branches(params, dts):
    return {dynamics_coefficients(*params, float(dt))[3] for dt in dts if dt}


def scan_case(n, params):
    """(targets (FRAMES, n) float32, dts, float32 coefficient table)"""
    rng = np.random.default_rng([n, PARAMS.index(tuple(params))])
    targets = np.abs(rng.standard_normal((FRAMES, n))).astype(np.float32)
    targets[HOLD[0]:HOLD[1]] = targets[HOLD[0]]
    dts = clock()
    return targets, dts, coeff_table(*params, dts, np.float32)


def oracle_f32(params, targets, dts, precision=PRECISION):
    """O.DynF32 from rest: values and derivatives of every frame, the final `previous`"""
    system = O.DynF32(targets.shape[1], *params, precision=precision)
    values, derivatives = np.empty_like(targets), np.empty_like(targets)
    for k in range(len(targets)):
        values[k] = system.step(np.ascontiguousarray(targets[k]), float(dts[k]))
        derivatives[k] = system.derivative
    return SimpleNamespace(values=values, derivatives=derivatives, previous=system.previous.copy())


@lru_cache(maxsize=None)
def scan_reference(n, params):
    """(targets, dts, coefficient table, oracle trajectory) of one float32 case: computed once, shared, and read only"""
    targets, dts, coeff = scan_case(n, params)
    oracle = oracle_f32(params, targets, dts)
    for array in (targets, dts, coeff, oracle.values, oracle.derivatives, oracle.previous):
        array.setflags(write=False)
    return targets, dts, coeff, oracle


def host_f32(params, targets, dts, precision=PRECISION):
    """The host class from rest, the target set before every step as ShaderSpectrogram.update does: value, target, previous, derivative and
    acceleration after every frame"""
    f, z, r = (float(p) for p in params)
    system = DynamicNumber(frequency=f, zeta=z, response=r, precision=precision, dtype=np.float32)
    system.set(np.zeros(targets.shape[1], np.float32))
    out = SimpleNamespace(**{name: np.empty_like(targets) for name in ("values", "targets", "previous", "derivatives", "accelerations")})
    with np.errstate(invalid="ignore"):
        for k in range(len(targets)):
            system.target = targets[k].copy()
            system.next(dt=abs(float(dts[k])))
            out.values[k], out.targets[k], out.previous[k] = system.value, system.target, system.previous
            out.derivatives[k], out.accelerations[k] = system.derivative, system.acceleration
    return out


def frozen_frames(values, dts, first, last):
    """Frames in [first, last) with dt != 0 whose values equal the frame before"""
    return [k for k in range(max(first, 1), last) if dts[k] and np.array_equal(values[k], values[k - 1], equal_nan=True)]


# ---- targets that are not finite ----------------------------------------------------------------------------------
NONFINITE_SIZES = (300, 200)         # the <1024, 2> instance and the one-wave instance
NONFINITE_KINDS = ("a", "b", "c")
NONFINITE_CASES = [(n, kind) for n in NONFINITE_SIZES for kind in NONFINITE_KINDS]
NONFINITE_PARAMS = (8, 1, 0)
NONFINITE_FRAMES = 120
NONFINITE_CALLS = (70, 50)           # the NaN arrives in the second call


def nonfinite_case(n, kind):
    """Targets held from row 5, so that by frame 80 every finite difference is within precision and the early-out hangs on the NaN alone.
    a: element 7 is NaN from frame 80 on. b: as a, and element 199 is -inf on frames 80 to 99 (two frames later target - value is
    -inf - -inf), then its held value again. c: every target is NaN from frame 80 on."""
    rng = np.random.default_rng([n, 7 + NONFINITE_KINDS.index(kind)])
    targets = np.abs(rng.standard_normal((NONFINITE_FRAMES, n))).astype(np.float32)
    targets[5:] = targets[5]
    if kind in ("a", "b"):
        targets[80:, 7] = np.nan
    if kind == "b":
        targets[80:100, 199] = -np.inf
    if kind == "c":
        targets[80:] = np.nan
    dts = clock(NONFINITE_FRAMES)
    return targets, dts, coeff_table(*NONFINITE_PARAMS, dts, np.float32)


# ---- the early-out at the precision itself -------------------------------------------------------------------------
EDGE_CASES = [(n, where) for n in (200, 300, 2050) for where in (0, n - 1)]      # one wave, <1024, 2>, <1024, 4>; first and last value
EDGE_PARAMS = (8, 1, 0)
EDGE_CALLS = (4, 4)


def precision_edge_case(n, where):
    """From rest, every target 0 but element `where`: the float32 just below the precision on frames 1 to 3 (max|target - value| < precision:
    the array stays frozen, `previous` included), the precision itself from frame 4 on (not below it: the array steps). A maximum that is
    off by one unit in the last place decides one of the two wrongly."""
    precision = np.float32(PRECISION)
    targets = np.zeros((sum(EDGE_CALLS), n), np.float32)
    targets[1:4, where] = np.nextafter(precision, np.float32(0))
    targets[4:, where] = precision
    dts = clock(len(targets))
    return targets, dts, coeff_table(*EDGE_PARAMS, dts, np.float32)


# ---- float64 scalar systems ---------------------------------------------------------------------------------------
F64_SYSTEMS = (2, 9, 64, 65, 130)
F64_CALLS = (63, 97)


def scalar_case(nsystems, with_nan=False):
    """System k takes PARAMS[k % 9], a start value and a target track of its own (held for 100 frames from a frame of its own, then
    released), so that the per-system early-out fires at different frames in different systems. `with_nan`: one more system, whose target
    is NaN from frame 80 on. Returns (params per system, start values, targets (FRAMES, systems) float64, dts, coefficients
    (systems, FRAMES, 4) float64)."""
    rng = np.random.default_rng([nsystems, int(with_nan)])
    count = nsystems + int(with_nan)
    params = [PARAMS[k % len(PARAMS)] for k in range(count)]
    starts = rng.uniform(-1.0, 1.0, count)
    targets = rng.uniform(-2.0, 2.0, (FRAMES, count))
    for k in range(count):
        first = 2 + k % 7
        targets[first:first + 100, k] = targets[first, k]
    if with_nan:
        targets[80:, -1] = np.nan
    dts = clock()
    coeff = np.stack([coeff_table(*p, dts, np.float64) for p in params])
    return params, starts, np.ascontiguousarray(targets), dts, np.ascontiguousarray(coeff)


def oracle_f64(params, start, targets, dts, integrate, precision=PRECISION):
    """O.DynF64 of one system: (FRAMES, 4) value, integral, derivative, previous after every frame"""
    system = O.DynF64(float(start), *params, integrate=bool(integrate), precision=precision)
    out = np.empty((len(targets), 4), np.float64)
    for k in range(len(targets)):
        system.step(float(targets[k]), float(dts[k]))
        out[k] = (system.value.value, system.integral.value, system.derivative.value, system.previous.value)
    return out


def host_f64(params, start, targets, dts, integrate, precision=PRECISION, float32_targets=False):
    """The host class of one scalar system: (FRAMES, 6) value, target, previous, derivative, acceleration, integral after every frame.
    `float32_targets`: the target is set as a numpy float32 scalar, as ShaderAudio.update sets the loudness targets."""
    f, z, r = (float(p) for p in params)
    system = DynamicNumber(value=float(start), frequency=f, zeta=z, response=r, integrate=bool(integrate), precision=precision)
    out = np.empty((len(targets), 6), np.float64)
    with np.errstate(invalid="ignore"):
        for k in range(len(targets)):
            system.target = np.float32(targets[k]) if float32_targets else float(targets[k])
            system.next(dt=abs(float(dts[k])))
            out[k] = (system.value, system.target, system.previous, system.derivative, system.acceleration, system.integral)
    return out
