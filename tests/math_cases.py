"""
The scalar built-ins of csrc/jit_runtime.hpp, value by value: the table of functions, their references and bounds, the inputs and the
GLSL probe that evaluates them. Shared by tests/test_host_math.py (x86 host build of the probe, CPU) and tests/test_gpu_math.py
(the gfx950 code object of the same translation). No GPU and no pytest in here.

References are of two kinds:
  * EXACT: the function's own formula restated in numpy float32 operations (every numpy float32 operation is one correctly rounded
    binary32 operation, as every operation of sfmath.hpp is): the bits must agree, NaN counting as equal to NaN. Where IEEE leaves the
    answer to the formula (mod(x, 0), smoothstep with e0 == e1, fract(-tiny) == 1) the restatement is the definition.
  * APPROX: a float64 numpy function, and a bound in ulp of the float32 rounding of the float64 value (`ulp_error`).

Every bound below carries the value it was derived from. All of them were measured on the x86 host build of the probe (HostFragment)
over `inputs()`; the device is held to the same bits by tests/test_gpu_math.py, so the figures are the device's too.

Integer results leave the fragment as two exact floats (the upper and the lower 16 bits): `intBitsToFloat` of a small negative int is
a NaN pattern, and NaNs compare equal here, so that route would pin nothing for int(-5.0). Booleans leave as 0 / 1.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

F = np.float32
WIDTH, HEIGHT = 256, 64                       # powers of two: gl_FragCoord = iResolution*astuv is exact, pixel (i, j) reads texel (i, j)
POINTS = WIDTH*HEIGHT
FLT_MAX, FLT_MIN, SUB_MIN, SUB_MAX = F(3.4028235e38), F(1.17549435e-38), F(1e-45), F(1.1754942e-38)
QNAN = np.array([0x7fc00000], np.uint32).view(F)[0]
SINCOS_REACH = F(2.0**20)                     # jit_runtime.hpp: at or below it sin/cos are sfmath's sequences, beyond it fmodf(x, TAU) first
ZERO_NEIGHBOURHOOD = 2.0**-25                 # a zero of sin/cos: |value| < |x|*2^-25 (see `circular_classes`)
ABSOLUTE_BOUND = 2.5e-7                       # the bound of test_sfmath_accuracy on |sin - want|, used next to the zeros


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(got, want) -> np.ndarray:
    """bit equality; a NaN equals a NaN"""
    got, want = np.asarray(got, F), np.asarray(want, F)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def ulp_error(got32, want64):
    """|got - want| in units of the spacing of float32 at the float32 rounding of want. Infinities stand for 2^128, the value float32
    overflows at, so that an overflow one step early or late is an error of a few ulp and inf against inf is none; NaN against NaN
    is none, NaN against a number is infinite."""
    got32, want64 = np.asarray(got32, F), np.asarray(want64, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        want32 = want64.astype(F)
        ulp = np.spacing(np.minimum(np.abs(want32), FLT_MAX)).astype(np.float64)
        ulp[ulp == 0] = np.finfo(F).tiny
        error = np.abs(np.clip(got32.astype(np.float64), -2.0**128, 2.0**128) - np.clip(want64, -2.0**128, 2.0**128))/ulp
    both_nan = np.isnan(got32) & np.isnan(want64)
    one_nan = np.isnan(got32) ^ np.isnan(want64)
    return np.where(both_nan, 0.0, np.where(one_nan, np.inf, error))


def floored_ulp_error(got32, want64):
    """ulp_error with the unit no smaller than ulp(1): an absolute floor around zero, for sinh and tanh, whose formulas subtract
    two values near 1 there and cannot do better than an ulp of those"""
    want64 = np.asarray(want64, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        unit = np.spacing(np.minimum(np.abs(want64.astype(F)), FLT_MAX)).astype(np.float64)
        scale = np.where(np.isnan(unit), 1.0, unit/np.maximum(unit, float(np.spacing(F(1.0)))))
        return ulp_error(got32, want64)*scale


# ---- the references ----------------------------------------------------------------------------------------------------------
def ref_round(x):
    f = np.floor(x)
    return np.where(x - f >= F(0.5), f + F(1.0), f).astype(F)


def ref_mod(x, y):
    return (x - y*np.floor(x/y)).astype(F)


def ref_min(a, b):
    return np.where(b < a, b, a).astype(F)


def ref_max(a, b):
    return np.where(a < b, b, a).astype(F)


def ref_clamp(x, lo, hi):
    return ref_min(ref_max(x, lo), hi)


def ref_mix(a, b, t):
    return (a*(F(1.0) - t) + b*t).astype(F)


def ref_smoothstep(e0, e1, x):
    t = ref_clamp((x - e0)/(e1 - e0), F(0.0), F(1.0))
    return (t*t*(F(3.0) - F(2.0)*t)).astype(F)


def ref_fma(a, b, c):
    """fmaf, correctly rounded: the product of two float32 is exact in float64; the sum is rounded to odd in float64 (Boldo-Melquiond:
    53 >= 2*24 + 2 bits) so that the final rounding to float32 is the only one that counts"""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    p = a*b
    s = p + c
    with np.errstate(invalid="ignore"):
        t = s - p
        e = (p - (s - t)) + (c - t)                                            # TwoSum: p + c = s + e exactly
    finite = np.isfinite(s) & (e != 0)
    raw = s.view(np.int64).copy()
    towards_zero = finite & ((e < 0) == (s > 0))                               # the exact sum is smaller in magnitude than s
    raw[towards_zero] -= 1
    raw[finite] |= 1
    return np.where(finite, raw.view(np.float64), s).astype(F)


def ref_to_int(x):
    """sfmath.hpp to_int: NaN -> 0, saturating, truncation otherwise"""
    x64 = np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=2.0**31, neginf=-2.0**31)
    return np.clip(np.trunc(x64), -2.0**31, 2.0**31 - 1).astype(np.int64).astype(np.int32)


def ref_to_uint(x):
    """jit_runtime.hpp to_uint: NaN and x <= 0 -> 0, saturating, truncation otherwise"""
    x64 = np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=2.0**32, neginf=0.0)
    return np.clip(np.trunc(x64), 0.0, 2.0**32 - 1).astype(np.int64).astype(np.uint32)


def _high(words):
    return (np.asarray(words).astype(np.int64) >> 16).astype(F)               # arithmetic shift for int32, logical for uint32


def _low(words):
    return (np.asarray(words).astype(np.int64) & 0xffff).astype(F)


def _bits_plus_one(x):
    return (bits(x).astype(np.int64) + 1).astype(np.uint32).view(F)


def _positive_zero(v):
    return np.asarray(v, np.float64) + 0.0                                     # -0 -> +0: GLSL gives a zero no direction


# ---- the table -----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    arity: int
    expr: str                                 # GLSL, in terms of the operands a, b, c
    kind: str                                 # "exact" | "approx"
    ref: Callable                             # exact: float32 arrays -> float32 bits; approx: float64 arrays -> float64 values
    bound: Optional[float] = None             # approx: ulp (see `unit`)
    measured: Optional[float] = None          # the largest error over inputs() on the x86 host build, in the same unit
    unit: str = "ulp"                         # "ulp" | "floored ulp" | "exp ulp": in units of (3 + 2|x|) ulp | "floored exp ulp"
    domain: Optional[Callable] = None         # operands -> bool mask of the points the bound covers; the rest is a named class
    outside: str = ""                         # … that class, in words: held to host = device (= oracle) bit equality only
    setup: str = ""                           # a GLSL statement the expression needs first
    oracle: Optional[tuple] = None            # (name in oracle.binding.MATH_FN, operands -> (a, b)), where the oracle has the function
    oracle_domain: Optional[Callable] = None  # points the oracle's sequence is the same on (default: all)


def _finite(*v):
    return np.logical_and.reduce([np.isfinite(x) for x in v])


def _circular(a):
    return np.abs(a) <= SINCOS_REACH


def _pow_domain(x, y):
    return (_finite(x, y) & (x > 0)) | ((x == 0) & ~np.isnan(y))


def _pow_ref(x, y):
    with np.errstate(all="ignore"):
        return np.power(np.abs(x), y)                                          # |x|: pow(-0, y) is pow(0, y) (sfmath: x == 0)


def _atan2_domain(y, x):
    return ~(np.isinf(y) & np.isinf(x)) & ~np.isnan(y) & ~np.isnan(x)


def _quiet(f):
    def wrapped(*v):
        with np.errstate(all="ignore"):
            return f(*v)
    return wrapped


RADIANS, DEGREES = F(np.float32(np.pi))/F(180.0), F(180.0)/F(np.float32(np.pi))       # the constants the header folds in float

CASES: list[Case] = [
    # -- exact kind
    Case("radians", 1, "radians(a)", "exact", _quiet(lambda a: a*RADIANS)),
    Case("degrees", 1, "degrees(a)", "exact", _quiet(lambda a: a*DEGREES)),
    Case("abs", 1, "abs(a)", "exact", lambda a: (bits(a) & 0x7fffffff).view(F)),
    Case("sign", 1, "sign(a)", "exact", lambda a: np.where(a > 0, F(1), np.where(a < 0, F(-1), F(0))).astype(F)),
    Case("floor", 1, "floor(a)", "exact", np.floor),
    Case("ceil", 1, "ceil(a)", "exact", np.ceil),
    Case("trunc", 1, "trunc(a)", "exact", np.trunc),
    Case("round", 1, "round(a)", "exact", _quiet(ref_round)),
    Case("roundEven", 1, "roundEven(a)", "exact", np.rint),
    Case("fract", 1, "fract(a)", "exact", _quiet(lambda a: a - np.floor(a))),
    Case("modf", 1, "part", "exact", _quiet(lambda a: a - np.trunc(a)), setup="float whole; float part = modf(a, whole);"),
    Case("modf.whole", 1, "whole", "exact", np.trunc, setup="float whole; float part = modf(a, whole);"),
    Case("isnan", 1, "isnan(a) ? 1.0 : 0.0", "exact", lambda a: np.isnan(a).astype(F)),
    Case("isinf", 1, "isinf(a) ? 1.0 : 0.0", "exact", lambda a: np.isinf(a).astype(F)),
    Case("int.high", 1, "float(ia >> 16)", "exact", lambda a: _high(ref_to_int(a)), setup="int ia = int(a);"),
    Case("int.low", 1, "float(ia & 65535)", "exact", lambda a: _low(ref_to_int(a)), setup="int ia = int(a);"),
    Case("uint.high", 1, "float((ua >> 16) & 65535)", "exact", lambda a: _high(ref_to_uint(a)), setup="int ua = int(uint(a));"),
    Case("uint.low", 1, "float(ua & 65535)", "exact", lambda a: _low(ref_to_uint(a)), setup="int ua = int(uint(a));"),
    Case("floatBitsToInt.high", 1, "float(ba >> 16)", "exact", lambda a: _high(bits(a).view(np.int32)), setup="int ba = floatBitsToInt(a);"),
    Case("floatBitsToInt.low", 1, "float(ba & 65535)", "exact", lambda a: _low(bits(a).view(np.int32)), setup="int ba = floatBitsToInt(a);"),
    Case("intBitsToFloat", 1, "intBitsToFloat(ba + 1)", "exact", _bits_plus_one, setup="int ba = floatBitsToInt(a);"),
    Case("sqrt", 1, "sqrt(a)", "exact", _quiet(np.sqrt), oracle=("sqrt", lambda a: (a, None))),
    Case("mod", 2, "mod(a, b)", "exact", _quiet(ref_mod), oracle=("mod", lambda a, b: (a, b))),
    Case("min", 2, "min(a, b)", "exact", ref_min),
    Case("max", 2, "max(a, b)", "exact", ref_max),
    Case("step", 2, "step(a, b)", "exact", lambda e, x: np.where(x < e, F(0), F(1)).astype(F)),
    # the forms of the two ternaries the oracle's test entry exposes
    Case("smoothstep(0, a, b)", 2, "smoothstep(0.0, a, b)", "exact", _quiet(lambda a, b: ref_smoothstep(np.zeros_like(a), a, b)),
         oracle=("smoothstep", lambda a, b: (a, b))),
    Case("mix(0.25, a, b)", 2, "mix(0.25, a, b)", "exact", _quiet(lambda a, b: ref_mix(np.full_like(a, 0.25), a, b)), oracle=("mix", lambda a, b: (a, b))),
    Case("clamp", 3, "clamp(a, b, c)", "exact", ref_clamp),
    Case("mix", 3, "mix(a, b, c)", "exact", _quiet(ref_mix)),
    Case("smoothstep", 3, "smoothstep(a, b, c)", "exact", _quiet(ref_smoothstep)),
    Case("fma", 3, "fma(a, b, c)", "exact", _quiet(ref_fma)),

    # -- approximate kind: the project's own 4 ulp (sfmath.hpp; the zeros of sin and cos: `circular_classes`)
    Case("sin", 1, "sin(a)", "approx", _quiet(np.sin), 4, 1.490, domain=_circular,
         outside="|x| > 2^20 = SINCOS_REACH: |sin| <= 1 and host = device only, no accuracy promised",
         oracle=("sin", lambda a: (a, None)), oracle_domain=lambda a: ~(np.abs(a) > SINCOS_REACH)),
    Case("cos", 1, "cos(a)", "approx", _quiet(np.cos), 4, 1.471, domain=_circular,
         outside="|x| > 2^20 = SINCOS_REACH: |cos| <= 1 and host = device only, no accuracy promised",
         oracle=("cos", lambda a: (a, None)), oracle_domain=lambda a: ~(np.abs(a) > SINCOS_REACH)),
    Case("atan", 1, "atan(a)", "approx", _quiet(np.arctan), 4, 2.545, oracle=("atan", lambda a: (a, None))),
    Case("atan2", 2, "atan(a, b)", "approx", _quiet(lambda y, x: np.arctan2(_positive_zero(y), _positive_zero(x))), 4, 2.882, domain=_atan2_domain,
         outside="both operands infinite (inf/inf: NaN), and a NaN operand, which sfmath's min and max may drop (atan(NaN, 0) = 0); pinned in test_host_math.py",
         oracle=("atan2", lambda a, b: (a, b))),
    Case("log2", 1, "log2(a)", "approx", _quiet(np.log2), 4, 1.907, oracle=("log2", lambda a: (a, None))),
    Case("log", 1, "log(a)", "approx", _quiet(np.log), 4, 2.009, oracle=("log", lambda a: (a, None))),
    Case("exp2", 1, "exp2(a)", "approx", _quiet(np.exp2), 4, 0.958, oracle=("exp2", lambda a: (a, None))),
    # -- GLSL's own allowance for exp (the precision table of the 4.x specifications: 3 + 2|x| ulp), the unit here: 0.544 of it at most,
    #    62.0 plain ulp at x = 87.3 (x*log2e is rounded before exp2 sees it)
    Case("exp", 1, "exp(a)", "approx", _quiet(np.exp), 1, 0.544, unit="exp ulp", oracle=("exp", lambda a: (a, None))),
    # -- nobody had fixed a number for these: the bound is the next power of two above the measured maximum. pow is exp2(y*log2(x)) and
    #    rounds the product like exp does: its 109.6 ulp are at x = 5.6e-6, y = -7.05 (|y*log2(x)| = 123), inside (0, 8] x [-8, 8]
    Case("tan", 1, "tan(a)", "approx", _quiet(np.tan), 4, 3.024, domain=lambda a: _circular(a) & ~circular_classes(a)[2],
         outside="|x| > 2^20, and the points next to a zero of sin or cos (`circular_classes`), where the quotient has no ulp bound"),
    Case("asin", 1, "asin(a)", "approx", _quiet(np.arcsin), 4, 3.118, domain=lambda a: ~(np.abs(a) > 1), outside="|x| > 1: undefined in GLSL"),
    Case("acos", 1, "acos(a)", "approx", _quiet(np.arccos), 4, 3.147, domain=lambda a: ~(np.abs(a) > 1), outside="|x| > 1: undefined in GLSL"),
    Case("pow", 2, "pow(a, b)", "approx", _pow_ref, 128, 109.636, domain=_pow_domain,
         outside="x < 0 (undefined in GLSL: NaN here), and an infinite or NaN operand, where exp2(y*log2(x)) is not IEEE pow (pow(inf, 0) = NaN)",
         oracle=("pow", lambda a, b: (a, b))),
    Case("inversesqrt", 1, "inversesqrt(a)", "approx", _quiet(lambda a: 1.0/np.sqrt(a)), 2, 1.394),
    # sinh and cosh are sums of two exp: in units of exp's allowance, 3 + 2|x| ulp (cosh: 7.87 plain ulp on |x| <= 10, 62.0 on |x| <= 88).
    # sinh and tanh subtract two values near 1 around zero: sinh(x) = 0 for |x| <= 2^-25, sinh(1e-4) is 2281 ulp off and tanh(1e-4) 440,
    # the absolute error staying below 2e-7 — their unit is floored at ulp(1). Pinned in test_host_math.py, not fixed.
    Case("sinh", 1, "sinh(a)", "approx", _quiet(np.sinh), 1, 0.544, unit="floored exp ulp", domain=lambda a: ~(np.abs(a) > 88),
         outside="|x| > 88: exp(|x|) is infinite before it is halved (sinh(89) = inf, true value 2.2e38)"),
    Case("cosh", 1, "cosh(a)", "approx", _quiet(np.cosh), 1, 0.544, unit="exp ulp", domain=lambda a: ~(np.abs(a) > 88),
         outside="|x| > 88: exp(|x|) is infinite before it is halved (cosh(89) = inf, true value 2.2e38)"),
    Case("tanh", 1, "tanh(a)", "approx", _quiet(np.tanh), 1, 0.894, unit="floored ulp"),
]
BY_NAME = {c.name: c for c in CASES}
ORACLE_FUNCTIONS = sorted({c.oracle[0] for c in CASES if c.oracle})


def circular_classes(x):
    """Which bound a circular input is held to. At a zero of sin or cos other than x = 0 the value is the reduced argument itself, and
    the first step of the Cody-Waite reduction, fmaf(-k, HI, x), rounds once a number of size k*(HI - pi/2) = |x|*(2/pi)*4.37e-8 =
    |x|*2^-25.1: an error of up to 2^-24 of that, which is an ulp of the value or more wherever |value| < |x|*2^-25. Those points are
    held to the absolute bound (2.5e-7); every other point, x near 0 included (k = 0, nothing to round), to the ulp bound.
    Returns (next to a zero of sin, next to a zero of cos, either)."""
    x64 = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        reduced = np.abs(x64) > np.pi/4
        near_sin = reduced & (np.abs(np.sin(x64)) < np.abs(x64)*ZERO_NEIGHBOURHOOD)
        near_cos = reduced & (np.abs(np.cos(x64)) < np.abs(x64)*ZERO_NEIGHBOURHOOD)
    return near_sin, near_cos, near_sin | near_cos


def error_of(case: Case, got, operands):
    """the error of an approximate case in its own unit, on every point (the caller masks with case.domain)"""
    want = case.ref(*[np.asarray(v, np.float64) for v in operands])
    error = floored_ulp_error(got, want) if case.unit.startswith("floored") else ulp_error(got, want)
    if case.unit.endswith("exp ulp"):
        error = error/(3.0 + 2.0*np.minimum(np.abs(np.nan_to_num(np.asarray(operands[0], np.float64), nan=0.0)), 1024.0))
    return error


def in_domain(case: Case, operands) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.ones(len(operands[0]), bool) if case.domain is None else case.domain(*[np.asarray(v, np.float64) for v in operands])


# ---- the inputs ------------------------------------------------------------------------------------------------------------------
def _signed(values):
    v = np.asarray(values, F)
    return np.concatenate([v, -v])


def _neighbours(centres, steps=2):
    c = np.asarray(centres, F)
    out = [c]
    up = down = c
    for _ in range(steps):
        up, down = np.nextafter(up, F(np.inf)), np.nextafter(down, F(-np.inf))
        out += [up, down]
    return np.concatenate(out)


SPECIALS = np.concatenate([
    _signed([0.0, SUB_MIN, SUB_MAX, FLT_MIN, 1.0, FLT_MAX, np.inf]), [QNAN],
    _signed([0.5, 1.5, 2.5, 0.49999997]),
    _signed([2.0**23 - 0.5, 2.0**23 + 1, 2.0**24 + 2]),
    _signed([2.0**31, 2.0**32]),
    _signed([2.0**31 - 128, 2.0**32 - 256, 2.0**22 + 0.5, 0.99999994, 65535.0, 65536.5])]).astype(F)
FEW = np.concatenate([_signed([0.0, SUB_MIN, FLT_MIN, 0.5, 1.0, 2.5, FLT_MAX, np.inf]), [QNAN]]).astype(F)      # for cubes of specials


def stratified(rng, per=32):
    """for each of the 254 normal exponents and the subnormal one, and each sign: `per` random mantissas"""
    exponent = np.repeat(np.arange(255, dtype=np.uint32), 2*per)
    sign = np.tile(np.repeat(np.array([0, 1], np.uint32), per), 255)
    mantissa = rng.integers(0, 1 << 23, exponent.size, dtype=np.uint32)
    return ((sign << 31) | (exponent << 23) | mantissa).astype(np.uint32).view(F)


def _pad(rows, rng, spread):
    """to whole 256 x 64 arrays, with everyday values"""
    rows = np.asarray(rows, F)
    missing = -len(rows) % POINTS
    return np.concatenate([rows, rng.uniform(-spread, spread, (missing, rows.shape[1])).astype(F)])


_cache: dict = {}


def inputs() -> dict:
    """{1: (n1, 1), 2: (n2, 2), 3: (n3, 3)} float32 operands by arity; n a multiple of 256*64. Deterministic."""
    if _cache:
        return _cache
    rng = np.random.default_rng(20260)
    u = lambda lo, hi, n: rng.uniform(lo, hi, n).astype(F)                     # noqa: E731
    half_pi = np.float64(np.pi)/2
    multiples = np.concatenate([np.arange(1, 65), 2**np.arange(7, 23)]).astype(np.float64)
    exponents = np.arange(-149, 128).astype(np.float64)
    unary = np.concatenate([
        SPECIALS,
        _signed(_neighbours((multiples*half_pi).astype(F))),                                  # the reduction of sin and cos
        _signed(_neighbours([np.tan(np.pi/8), 1.0])),                                        # atan's two splits
        _neighbours((np.sqrt(2.0)*2.0**exponents[:-1]).astype(F)),                            # log2's mantissa split, every binade
        _neighbours([-150.0, -149.5, -149.0, -126.0, -125.5, 127.0, 127.5, np.nextafter(F(128), F(0)), 128.0]),   # exp2's ends
        _signed(_neighbours(np.array([-150, -149.5, -149, -126, -125.5, 127, 127.5, 128])/np.log2(np.e))),        # … seen through exp
        _signed(np.concatenate([np.arange(0, 40) + 0.5, 2.0**np.arange(1, 24) + 0.5, 2.0**np.arange(1, 24) - 0.5])),   # ties of rintf and round
        _signed(_neighbours([88.0, 89.0, 2.0**20, 10.0, 2.0**-25, 1e-4])),
        stratified(rng),
        u(-8, 8, 16384), u(-2.0**20, 2.0**20, 16384),                                       # the circular functions' everyday domain
        u(-1, 1, 8192), u(-88, 88, 8192), u(-10, 10, 8192), u(0, 8, 4096),
    ]).astype(F)
    _cache[1] = _pad(unary[:, None], rng, 4.0)

    s = stratified(rng)
    grid = np.stack(np.meshgrid(SPECIALS, SPECIALS, indexing="ij"), -1).reshape(-1, 2)
    binary = np.concatenate([
        grid,
        np.stack([s, rng.permutation(stratified(rng))], 1),
        np.stack([s, u(-8, 8, s.size)], 1), np.stack([u(-8, 8, s.size), s], 1),
        np.stack([u(0, 8, 16384), u(-8, 8, 16384)], 1),                                     # pow's everyday domain (0, 8] x [-8, 8]
        np.stack([np.exp(u(-30, 30, 4096)), u(-6, 6, 4096)], 1),                            # … and bases far from 1
        np.stack([u(-3, 3, 8192), u(-3, 3, 8192)], 1),                                      # atan(y, x) around the circle
        np.stack([u(-100, 100, 4096), u(-10, 10, 4096)], 1),                                # mod
        np.stack([u(-4, 4, 512), np.zeros(512, F)], 1), np.stack([np.zeros(512, F), u(-4, 4, 512)], 1),      # x = 0, y = 0
        np.stack([np.arange(-256, 256)*F(0.75), np.full(512, 0.75, F)], 1),                 # exact multiples for mod
    ]).astype(F)
    _cache[2] = _pad(binary, rng, 4.0)

    cube = np.stack(np.meshgrid(FEW, FEW, FEW, indexing="ij"), -1).reshape(-1, 3)
    slots = []
    for slot in range(3):                                                                   # every special in every slot, everyday values around it
        block = rng.uniform(-2, 2, (len(SPECIALS)*8, 3)).astype(F)
        block[:, slot] = np.repeat(SPECIALS, 8)
        slots.append(block)
    edge = u(-4, 4, 1024)
    t = stratified(rng)
    ternary = np.concatenate([
        cube, *slots,
        np.stack([t, rng.permutation(stratified(rng)), rng.permutation(stratified(rng))], 1),
        np.stack([edge, edge, u(-8, 8, 1024)], 1),                                          # smoothstep with e0 == e1 (and clamp with lo == hi)
        np.stack([edge, edge, edge], 1),
        rng.uniform(-4, 4, (8192, 3)).astype(F),
        np.stack([u(0, 1, 4096), u(1, 2, 4096), u(-1, 3, 4096)], 1),                        # edges in order, x on both sides
    ]).astype(F)
    _cache[3] = _pad(ternary, rng, 4.0)
    return _cache


def pack(operands: np.ndarray) -> np.ndarray:
    """(n, arity) operands -> (n/POINTS, HEIGHT, WIDTH, 4) RGBA32F arrays: operands in the first channels, zeros between, and the
    first operand in reverse order in the spare fourth channel, so that the echo covers all four channels"""
    n, arity = operands.shape
    texels = np.zeros((n, 4), F)
    texels[:, :arity] = operands
    texels[:, 3] = operands[::-1, 0]
    return texels.reshape(n//POINTS, HEIGHT, WIDTH, 4)


# ---- the probe fragment ----------------------------------------------------------------------------------------------------------
def groups() -> list[list[Case]]:
    """group 0 is the echo; then the cases four to a group, in table order, one arity per group"""
    out: list[list[Case]] = [[]]
    for arity in (1, 2, 3):
        cases = [c for c in CASES if c.arity == arity]
        out += [cases[k:k + 4] for k in range(0, len(cases), 4)]
    return out


def probe_glsl() -> str:
    lines = ["uniform int group;", "void main() {",
             "    vec4 t = texelFetch(operands, ivec2(gl_FragCoord.xy), 0);",
             "    float a = t.x; float b = t.y; float c = t.z;",
             "    vec4 r = vec4(0.0);",
             "    switch (group) {",
             "        case 0: r = t; break;"]
    for index, cases in enumerate(groups()):
        if index == 0:
            continue
        setups = list(dict.fromkeys(c.setup for c in cases if c.setup))
        results = [c.expr for c in cases] + ["0.0"]*(4 - len(cases))
        lines.append(f"        case {index}: {{ {' '.join(setups)} r = vec4({', '.join(results)}); break; }}")
    for offset, name in enumerate(VECTOR_FORMS):
        lines.append(f"        case {len(groups()) + offset}: r = {name}(t); break;")
    lines += ["        default: break;", "    }", "    fragColor = r;", "}"]
    return "\n".join(lines) + "\n"


PROBE_UNIFORMS = [("sampler2D", "operands")]
VECTOR_FORMS = ["round", "sin", "cos", "tan"]     # the vec4 forms of what this file's fixes touch: they must go through the scalar ones


def evaluate(render: Callable[[int, np.ndarray], np.ndarray]) -> tuple[dict, dict]:
    """Run every group over its inputs. `render(group, texels)` shades one (HEIGHT, WIDTH, 4) float32 array of operands with the
    probe and returns the (HEIGHT, WIDTH, 4) float32 target. Returns ({case name: (n,) results}, {arity: (n, 4) echo of group 0})."""
    results, echo = {}, {}
    data = inputs()
    for arity in (1, 2, 3):
        arrays = pack(data[arity])
        echo[arity] = np.concatenate([render(0, texels).reshape(-1, 4) for texels in arrays])
        for index, cases in enumerate(groups()):
            if index == 0 or cases[0].arity != arity:
                continue
            out = np.concatenate([render(index, texels).reshape(-1, 4) for texels in arrays])
            for channel, case in enumerate(cases):
                results[case.name] = np.ascontiguousarray(out[:, channel])
        if arity == 1:
            for offset, name in enumerate(VECTOR_FORMS):
                results[f"vec4 {name}"] = np.concatenate([render(len(groups()) + offset, texels).reshape(-1, 4) for texels in arrays])
    return results, echo


def operands_of(case: Case) -> list[np.ndarray]:
    data = inputs()[case.arity]
    return [np.ascontiguousarray(data[:, k]) for k in range(case.arity)]


def describe(case: Case, wrong: np.ndarray, got, want, limit=8) -> str:
    """count, function, operands and both values in hex for the first points of `wrong`"""
    operands = operands_of(case)
    where = np.flatnonzero(wrong)
    rows = [f"{case.name}: {len(where)} of {len(wrong)} points differ"]
    for k in where[:limit]:
        args = ", ".join(f"{float(v[k])!r} [{int(bits(v[k:k + 1])[0]):08x}]" for v in operands)
        rows.append(f"  {case.expr} at ({args}): got {float(got[k])!r} [{int(bits(got[k:k + 1])[0]):08x}], want {float(want[k])!r} [{int(bits(np.asarray(want[k:k + 1], F))[0]):08x}]")
    return "\n".join(rows)


# ---- the checks, shared by the host and the device tests ------------------------------------------------------------------------
def check_echo(echo: dict) -> None:
    """group 0 returns the four channels it fetched, bit for bit — subnormals, infinities and the NaN's payload included: float
    textures and float targets carry every value unharmed, and pixel (i, j) is fed operand (i, j)"""
    for arity, operands in inputs().items():
        sent = pack(operands).reshape(-1, 4)
        wrong = bits(echo[arity]) != bits(sent)
        assert not wrong.any(), f"arity {arity}: {int(wrong.sum())} of {wrong.size} echoed floats differ; first at {np.argwhere(wrong)[0].tolist()}: " \
                                f"{int(bits(echo[arity])[tuple(np.argwhere(wrong)[0])]):08x} for {int(bits(sent)[tuple(np.argwhere(wrong)[0])]):08x}"


def check_same(results: dict, others: dict, what: str) -> None:
    """two evaluations of the probe agree bit for bit on every point of every case (NaN = NaN)"""
    failures = [f"vec4 {name}" for name in VECTOR_FORMS if not same_bits(results[f"vec4 {name}"], others[f"vec4 {name}"]).all()]
    for case in CASES:
        wrong = ~same_bits(results[case.name], others[case.name])
        if wrong.any():
            failures.append(describe(case, wrong, results[case.name], others[case.name]))
    assert not failures, f"{what}:\n" + "\n".join(failures)


def check_exact(results: dict) -> None:
    failures = []
    for case in CASES:
        if case.kind != "exact":
            continue
        want = np.asarray(case.ref(*operands_of(case)), F)
        wrong = ~same_bits(results[case.name], want)
        if wrong.any():
            failures.append(describe(case, wrong, results[case.name], want))
    assert not failures, "\n".join(failures)


def measure(results: dict) -> dict:
    """{case name: largest error in the case's unit over its domain} — for sin and cos over the points held to the ulp bound"""
    out = {}
    for case in CASES:
        if case.kind != "approx":
            continue
        operands = operands_of(case)
        covered = in_domain(case, operands)
        if case.name in ("sin", "cos"):
            covered &= ~circular_classes(operands[0])[0 if case.name == "sin" else 1]
        out[case.name] = float(error_of(case, results[case.name], operands)[covered].max())
    return out


def check_approx(results: dict, report=print) -> None:
    measured = measure(results)
    failures = []
    for case in CASES:
        if case.kind != "approx":
            continue
        report(f"{case.name:12s} {measured[case.name]:10.3f} {case.unit} (bound {case.bound}, recorded {case.measured})")
        if not measured[case.name] <= case.bound:
            operands = operands_of(case)
            error = error_of(case, results[case.name], operands)
            worst = int(np.argmax(np.where(in_domain(case, operands), error, -1.0)))
            failures.append(f"{case.name}: {measured[case.name]:.3f} {case.unit} > {case.bound} at ({', '.join(repr(float(v[worst])) for v in operands)}): "
                            f"got {float(results[case.name][worst])!r}")
    assert not failures, "\n".join(failures)


def check_circular(results: dict, report=print) -> None:
    """sin and cos on |x| <= 2^20: 2.5e-7 absolute on every point; 4 ulp (check_approx) on every point but those next to a zero, which
    must be under 1 % of the circular inputs"""
    x = operands_of(BY_NAME["sin"])[0]
    inside = in_domain(BY_NAME["sin"], [x])
    x64 = x.astype(np.float64)
    classes = circular_classes(x)
    for which, (name, f) in enumerate((("sin", np.sin), ("cos", np.cos))):
        with np.errstate(all="ignore"):
            error = np.abs(results[name].astype(np.float64) - f(x64))
        share = float((classes[which] & inside).sum()/inside.sum())
        report(f"{name}: largest absolute error on |x| <= 2^20 {error[inside].max():.3g}; {int((classes[which] & inside).sum())} of {int(inside.sum())} "
               f"points ({100*share:.2f} %) are next to a zero and held to it alone")
        assert error[inside].max() <= ABSOLUTE_BOUND, (name, float(error[inside].max()), float(x[inside][np.argmax(error[inside])]))
        assert share < 0.01, (name, share)


def check_properties(results: dict) -> None:
    """what holds on every finite input, whatever its size"""
    x = operands_of(BY_NAME["sin"])[0]
    finite = np.isfinite(x)
    for name in ("sin", "cos"):
        wrong = finite & ~(np.abs(results[name]) <= 1)
        assert not wrong.any(), describe(BY_NAME[name], wrong, results[name], np.clip(results[name], -1, 1))
        assert np.isnan(results[name][~finite]).all(), name
    r = results["round"]
    x64, r64 = np.where(finite, x, 0).astype(np.float64), np.where(finite, r, 0).astype(np.float64)
    wrong = finite & ~((r64 == np.floor(r64)) & (np.abs(r64 - x64) <= 0.5))
    assert not wrong.any(), describe(BY_NAME["round"], wrong, r, np.floor(x64 + 0.5).astype(F))
    wrong = finite & (r64 != np.floor(x64 + 0.5))                                # halves towards +inf: floor(x + 1/2), exact in float64
    assert not wrong.any(), describe(BY_NAME["round"], wrong, r, np.floor(x64 + 0.5).astype(F))
    large = finite & (np.abs(x) >= F(2.0**23))
    assert large.sum() > 1000 and np.array_equal(r[large], x[large])
    fract = results["fract"]
    assert ((fract[finite] >= 0) & (fract[finite] <= 1)).all()
    assert np.array_equal(results["isnan"], np.isnan(x).astype(F)) and np.array_equal(results["isinf"], np.isinf(x).astype(F))
    assert results["isnan"].sum() >= 1 and results["isinf"].sum() >= 2


def check_vector_forms(results: dict) -> None:
    """`round(vec4)`, `sin(vec4)` … of the texel (a, 0, 0, a in reverse order) are the scalar forms component by component"""
    for name in VECTOR_FORMS:
        scalar, vector = results[name], results[f"vec4 {name}"]
        assert same_bits(vector[:, 0], scalar).all() and same_bits(vector[:, 3], scalar[::-1]).all(), name
        assert same_bits(vector[:, 1], np.full(len(scalar), scalar[np.flatnonzero(bits(operands_of(BY_NAME[name])[0]) == 0)[0]])).all(), name


_oracle: dict = {}


def oracle_values() -> dict:
    """{case name: the oracle's values on the case's inputs} for the cases oracle/sfo_math.h has (computed once per session)"""
    if not _oracle:
        from oracle import binding as O
        for case in CASES:
            if case.oracle:
                name, arrange = case.oracle
                a, b = arrange(*operands_of(case))
                _oracle[case.name] = O.math(name, a, 0.0 if b is None else b)
    return _oracle


def check_oracle(results: dict) -> None:
    """bit equality with oracle/sfo_math.h wherever it has the function. sin and cos: for |x| <= SINCOS_REACH (and the non-finite
    inputs) — the oracle's sequence is sfmath's, which the wrappers of jit_runtime.hpp leave alone there: this is also the proof that
    the wrapper changed no bit at or below the reach"""
    failures = []
    for case in CASES:
        if not case.oracle:
            continue
        want = oracle_values()[case.name]
        covered = np.ones(len(want), bool) if case.oracle_domain is None else case.oracle_domain(*operands_of(case))
        wrong = covered & ~same_bits(results[case.name], want)
        if wrong.any():
            failures.append(describe(case, wrong, results[case.name], want))
    assert not failures, "\n".join(failures)
