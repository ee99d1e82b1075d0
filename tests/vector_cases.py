"""
The vector, matrix and integer built-ins of csrc/jit_runtime.hpp, value by value: the table of rows, their references and bounds, the
inputs and the GLSL probes that evaluate them. Shared by tests/test_host_vector.py (x86 host build of the probes, CPU) and
tests/test_gpu_vector.py (the gfx950 code objects of the same translations). No GPU and no pytest in here. The helpers (bit equality,
specials, stratified sweeps) are those of tests/math_cases.py, which holds the scalar built-ins the same way.

A probe reads four RGBA32F operand textures A, B, C, D of 256 x 64 (sixteen floats per point) and writes one vec4. `uniform int group`
picks the row, `uniform int column` the part of a result wider than four floats (a matrix column, or two of four integer words). Group 0
echoes the operands. Integer operands and results travel as two exact floats per 32-bit word (upper and lower 16 bits).

Every row has a reference of the EXACT kind: either the header's formula restated in numpy float32 operations in the written order
(-ffp-contract=off: the bits must agree, NaN = NaN), int32/uint32 arithmetic restated in int64 and masked, or — for the component-wise
forms — the scalar form's own result at that component (`like`). Float rows built from sums of products also have a float64 WITNESS
with a derived bound (`gamma`), on the points where every operand is zero or within 2^-30 .. 2^30 (no product of up to four of them
leaves the normal range); at least 90 % of a row's everyday points must lie inside that mask.

refract's witness is a running error bound (`Bounded`) on the points where the float64 k is safely negative (the zero vector, exactly) or
at least 2^-6; the neighbourhood of k = 0, the float neighbours of the critical eta included, is held by the restatement. The prelude functions that call sin / cos / atan / exp equal the composition of
the probe's own scalar results with float32 operations; angle is the float32 quotient through the header's acos composition, hsv2rgb its formula (no transcendental in it); the noise
functions are held to device = host and to [0, 1).

Pinned as this implementation's definition, by restatement: length/distance are sqrt(dot) (inf where the sum of squares overflows, 0
where it underflows), normalize(0) is NaN, a singular inverse is inf/NaN, integer / and % are C's (truncation, the dividend's sign),
abs(INT_MIN) is INT_MIN.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from tests import math_cases as M

F = M.F
WIDTH, HEIGHT, POINTS = M.WIDTH, M.HEIGHT, M.POINTS
U = 2.0**-24
MASK32 = (1 << 32) - 1
SW = {1: ".x", 2: ".xy", 3: ".xyz", 4: ""}
VEC = {1: "float", 2: "vec2", 3: "vec3", 4: "vec4"}


def gamma(k: int) -> float:
    return k*U/(1 - k*U)


def quiet(f):
    def wrapped(*v):
        with np.errstate(all="ignore"):
            return f(*v)
    return wrapped


@dataclass
class Row:
    name: str
    fragment: str                             # which probe
    body: str                                 # GLSL: sets `r` (kind vec), `matN R` (kind matN) or `uvec4 R` (kind words)
    inputs: str                               # the operand set
    ref: Optional[Callable] = None            # X (n, 16) float32 | W (n, 8) int64 words -> (n, width) float32 | int64 words
    like: Optional[str] = None                # the row whose first `width` results these must equal (the scalar form)
    width: int = 4                            # the result's scalars; the rest of the target is zero
    kind: str = "vec"                         # "vec" | "mat2" | "mat3" | "mat4" | "words"
    witness: Optional[Callable] = None        # (X, got (n, width)) -> (error, bound): float64 arrays, same shape
    note: str = ""
    size: tuple = (WIDTH, HEIGHT)
    uses: tuple = ()                          # rows of the same probe whose results the reference composes: ref(X, *their values)
    within: Optional[tuple] = None            # [lo, hi) every result lies in on the everyday points (the chaotic rows; fract(-tiny) is 1, sin(inf) NaN)

    @property
    def columns(self) -> int:
        return {"vec": 1, "mat2": 2, "mat3": 3, "mat4": 4, "words": 2}[self.kind]


ROWS: list[Row] = []


def wrap(n: int, e: str) -> str:
    return {1: f"vec4({e}, 0.0, 0.0, 0.0)", 2: f"vec4({e}, 0.0, 0.0)", 3: f"vec4({e}, 0.0)", 4: e}[n]


def wrap_words(n: int, e: str) -> str:
    return {1: f"uvec4({e}, 0u, 0u, 0u)", 2: f"uvec4({e}, 0u, 0u)", 3: f"uvec4({e}, 0u)", 4: e}[n]


def part(X, letter: str, n: int = 4):
    k = "ABCD".index(letter)*4
    return X[:, k:k + n]


# ---- float vectors: component-wise forms -----------------------------------------------------------------------------------------
MAP1 = ("radians degrees sin cos tan asin acos atan exp log exp2 log2 sqrt inversesqrt sinh cosh tanh abs sign floor ceil trunc round "
        "roundEven fract").split()


def componentwise(name: str, arguments: str, exact: Optional[Callable]) -> None:
    """`arguments`: one letter per argument, upper case for a vector (A, B, C), lower case for that texture's .x as a scalar. The
    scalar row evaluates the function once per component; the vecN rows must equal it component by component."""
    label = f"{name}({', '.join('genType' if a.isupper() else 'float' for a in arguments)})"
    scalar = ", ".join(f"{name}({', '.join(f'{a.upper()}.{c}' if a.isupper() else f'{a.upper()}.x' for a in arguments)})" for c in "xyzw")
    ref = None
    if exact is not None:
        ref = quiet(lambda X: exact(*[part(X, a.upper()) if a.isupper() else part(X, a.upper(), 1) for a in arguments]))
    ROWS.append(Row(f"{label} per component", "float", f"r = vec4({scalar});", "vec", ref=ref,
                    note="" if exact else "scalar form bounded in math_cases: device = host here"))
    for n in (2, 3, 4):
        call = f"{name}({', '.join(f'{a}{SW[n]}' if a.isupper() else f'{a.upper()}.x' for a in arguments)})"
        ROWS.append(Row(label.replace("genType", VEC[n]), "float", f"r = {wrap(n, call)};", "vec", like=f"{label} per component", width=n))


def _exact(name):
    case = M.BY_NAME[name]
    return case.ref if case.kind == "exact" else None


def ref_acos(x):
    """jit_runtime.hpp: acos(x) = atan(sqrt((1 - x)(1 + x)), x). The products and sqrt are float32 operations; atan(y, x) is the
    oracle's restatement of sfmath's sequence, which math_cases holds to the host's and the device's bits on every input"""
    from oracle import binding as O
    x = np.ascontiguousarray(x, F)
    with np.errstate(all="ignore"):
        y = np.sqrt((F(1.0) - x)*(F(1.0) + x))
    return O.math("atan2", y.reshape(-1), x.reshape(-1)).reshape(x.shape)


for _f in MAP1:
    componentwise(_f, "A", ref_acos if _f == "acos" else _exact(_f))
for _f in ("atan", "pow", "mod", "min", "max", "step"):
    componentwise(_f, "AB", _exact(_f))
for _f in ("mod", "min", "max"):
    componentwise(_f, "Ab", _exact(_f))
componentwise("step", "bA", _exact("step"))
componentwise("clamp", "ABC", M.ref_clamp)
componentwise("clamp", "Abc", M.ref_clamp)
componentwise("mix", "ABC", M.ref_mix)
componentwise("mix", "ABc", M.ref_mix)
componentwise("smoothstep", "ABC", M.ref_smoothstep)
componentwise("smoothstep", "abC", M.ref_smoothstep)
componentwise("fma", "ABC", M.ref_fma)

for _n in (1, 2, 3, 4):
    _t, _s = VEC[_n], SW[_n]
    _sel = f"lessThan(C{_s}, {_t}(0.0))" if _n > 1 else "C.x < 0.0"
    ROWS.append(Row(f"mix({_t}, {_t}, b{_t if _n > 1 else 'ool'})", "float", f"r = {wrap(_n, f'mix(A{_s}, B{_s}, {_sel})')};", "vec",
                    ref=lambda X, n=_n: np.where(part(X, "C", n) < 0, part(X, "B", n), part(X, "A", n)), width=_n))
    ROWS.append(Row(f"modf({_t}) part", "float", f"{_t} w; {_t} p = modf(A{_s}, w); r = {wrap(_n, 'p')};", "vec",
                    ref=quiet(lambda X, n=_n: part(X, "A", n) - np.trunc(part(X, "A", n))), width=_n))
    ROWS.append(Row(f"modf({_t}) whole", "float", f"{_t} w; {_t} p = modf(A{_s}, w); r = {wrap(_n, 'w')};", "vec",
                    ref=lambda X, n=_n: np.trunc(part(X, "A", n)), width=_n))
    if _n > 1:
        ROWS.append(Row(f"isnan({_t})", "float", f"r = {wrap(_n, f'{_t}(isnan(A{_s}))')};", "vec", ref=lambda X, n=_n: np.isnan(part(X, "A", n)).astype(F), width=_n))
        ROWS.append(Row(f"isinf({_t})", "float", f"r = {wrap(_n, f'{_t}(isinf(A{_s}))')};", "vec", ref=lambda X, n=_n: np.isinf(part(X, "A", n)).astype(F), width=_n))


# ---- geometric functions: restatements generic over the number type and over what a subtraction is --------------------------------
def minus(a, b):
    return a - b


def plus(a, b):
    return a + b


def dot_(a, b):
    s = a[0]*b[0]
    for k in range(1, len(a)):
        s = s + a[k]*b[k]
    return s


def cross_(a, b, sub=minus):
    return [sub(a[1]*b[2], b[1]*a[2]), sub(a[2]*b[0], b[2]*a[0]), sub(a[0]*b[1], b[0]*a[1])]


def comps(X, letter, n, dtype=F):
    return [part(X, letter, n)[:, k].astype(dtype) for k in range(n)]


def stack(v):
    return np.stack([np.broadcast_to(c, v[0].shape) for c in v], 1)


def ref_length(a):
    return np.sqrt(dot_(a, a))


def ref_refract(i, n, eta):
    c = dot_(n, i)
    k = F(1.0) - eta*eta*(F(1.0) - c*c)
    root = np.sqrt(np.where(k < 0, F(0.0), k))
    return [np.where(k < 0, F(0.0), eta*i[j] - (eta*c + root)*n[j]).astype(F) for j in range(len(i))], k


def ordinary(X, slots) -> np.ndarray:
    """the witness mask: every operand the row reads is zero or within 2^-30 .. 2^30, so that no float64 intermediate (a product of
    up to four operands, sums of such) is infinite, NaN or below the normal range of float32"""
    v = np.abs(X[:, slots].astype(np.float64))
    return (np.isfinite(v) & ((v == 0) | ((v >= 2.0**-30) & (v <= 2.0**30)))).all(1)


def witness_terms(exact: Callable, k: int, slots):
    """|got - exact| <= gamma_k * sum|terms|: `exact(X64, sub)` is the formula in float64; with |operands| and every subtraction an
    addition it is the sum of the absolute values of its expanded products"""
    def check(X, got):
        X64 = X.astype(np.float64)
        with np.errstate(all="ignore"):
            want = stack(exact(X64, minus))
            terms = stack(exact(np.abs(X64), plus))
            error = np.abs(got.astype(np.float64) - want)
        return error, gamma(k)*terms, ordinary(X, slots) & np.isfinite(want).all(1)
    return check


def witness_relative(exact: Callable, bound: float, slots):
    def check(X, got):
        with np.errstate(all="ignore"):
            want = stack(exact(X.astype(np.float64)))
            error = np.abs(got.astype(np.float64) - want)
        return error, bound*np.abs(want), ordinary(X, slots) & np.isfinite(want).all(1)      # (normalize(0): 0/0 in float64 too)
    return check


class Bounded:
    """a float64 value of the exact formula with a bound on what the float32 evaluation of the same formula can be off by: every
    float32 operation returns (x op y)(1 + d), |d| <= u, so an error e_x, e_y of the operands becomes
    (e_x + e_y)(1 + u) + u|z| after + and -, (|x| e_y + |y| e_x + e_x e_y)(1 + u) + u|z| after *, and
    e_x/(sqrt(x) + sqrt(x - e_x))(1 + u) + u sqrt(x) after sqrt (x - e_x > 0). Expanded to first order this is gamma_k * sum|terms|."""
    def __init__(self, v, e=0.0):
        self.v, self.e = np.asarray(v, np.float64), np.asarray(e, np.float64) + 0.0*np.asarray(v, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, Bounded) else Bounded(x)

    def __add__(self, o):
        o = Bounded.of(o)
        z = self.v + o.v
        return Bounded(z, (self.e + o.e)*(1 + U) + U*np.abs(z))

    def __sub__(self, o):
        o = Bounded.of(o)
        z = self.v - o.v
        return Bounded(z, (self.e + o.e)*(1 + U) + U*np.abs(z))

    def __rsub__(self, o):
        return Bounded.of(o) - self

    def __mul__(self, o):
        o = Bounded.of(o)
        z = self.v*o.v
        return Bounded(z, (np.abs(self.v)*o.e + np.abs(o.v)*self.e + self.e*o.e)*(1 + U) + U*np.abs(z))

    __rmul__ = __mul__

    def sqrt(self):
        root = np.sqrt(np.maximum(self.v, 0.0))
        return Bounded(root, self.e/(root + np.sqrt(np.maximum(self.v - self.e, 0.0)))*(1 + U) + U*root)


REFRACT_ROOT_FLOOR = 2.0**-6                  # the witness of the refracted branch covers k >= this; below it sqrt amplifies k's error without bound


def witness_refract(n: int):
    """k in float64 alone decides the branch. Where k + e_k < 0 the float32 k is negative too: the result must be the zero vector
    exactly (bound 0). Where k >= 2^-6 and k - e_k > 0 the refracted vector keeps the running bound of `Bounded` (times 1.001 for the
    float64 arithmetic of the bound itself). In between — the neighbourhood of k = 0 — the restatement alone holds the row."""
    slots = _slots("AB", n) + [12]

    def check(X, got):
        with np.errstate(all="ignore"):
            i, normal, eta = [Bounded(v) for v in comps(X, "A", n, np.float64)], [Bounded(v) for v in comps(X, "B", n, np.float64)], Bounded(X[:, 12].astype(np.float64))
            c = dot_(normal, i)
            k = 1.0 - eta*eta*(1.0 - c*c)
            reflected, refracted = (k.v + k.e < 0), (k.v >= REFRACT_ROOT_FLOOR) & (k.v - k.e > 0)
            scale = eta*c + k.sqrt()
            out = [eta*p - scale*q for p, q in zip(i, normal)]
            want = np.where(reflected[:, None], 0.0, stack([o.v for o in out]))
            bound = np.where(reflected[:, None], 0.0, 1.001*stack([o.e for o in out]))
            error = np.abs(got.astype(np.float64) - want)
        return error, bound, ordinary(X, slots) & (reflected | refracted) & np.isfinite(want).all(1)
    return check


def _slots(letters: str, n: int, extra=()):
    return [("ABCD".index(c))*4 + k for c in letters for k in range(n)] + list(extra)


for _n in (1, 2, 3, 4):
    _t, _s = VEC[_n], SW[_n]
    a_ = lambda X, n=_n, d=F: comps(X, "A", n, d)                                                  # noqa: E731
    b_ = lambda X, n=_n, d=F: comps(X, "B", n, d)                                                  # noqa: E731
    c_ = lambda X, n=_n, d=F: comps(X, "C", n, d)                                                  # noqa: E731
    if _n == 1:                                   # the scalar forms: |x|, |a - b|, a*b, sign(x)
        ROWS.append(Row("length(float)", "geometric", f"r = {wrap(1, 'length(A.x)')};", "vec", ref=lambda X: np.abs(part(X, "A", 1)), width=1))
        ROWS.append(Row("distance(float)", "geometric", f"r = {wrap(1, 'distance(A.x, B.x)')};", "vec", ref=quiet(lambda X: np.abs(part(X, "A", 1) - part(X, "B", 1))), width=1))
        ROWS.append(Row("dot(float)", "geometric", f"r = {wrap(1, 'dot(A.x, B.x)')};", "vec", ref=quiet(lambda X: part(X, "A", 1)*part(X, "B", 1)), width=1))
        ROWS.append(Row("normalize(float)", "geometric", f"r = {wrap(1, 'normalize(A.x)')};", "vec", ref=lambda X: M.BY_NAME["sign"].ref(part(X, "A", 1)), width=1))
    _vector_forms = [Row(f"dot({_t})", "geometric", f"r = {wrap(1, f'dot(A{_s}, B{_s})')};", "vec", width=1,
                    ref=quiet(lambda X, a=a_, b=b_: stack([dot_(a(X), b(X))])),
                    witness=witness_terms(lambda X, sub, a=a_, b=b_: [dot_(a(X, d=np.float64), b(X, d=np.float64))], _n, _slots("AB", _n))),
                     Row(f"length({_t})", "geometric", f"r = {wrap(1, f'length(A{_s})')};", "vec", width=1,
                    ref=quiet(lambda X, a=a_: stack([ref_length(a(X))])),
                    witness=witness_relative(lambda X, a=a_: [np.sqrt(dot_(a(X, d=np.float64), a(X, d=np.float64)))], (gamma(_n)/2 + U)*1.001, _slots("A", _n)),
                    note="sqrt(dot): inf where the sum of squares overflows, 0 where it underflows"),
                     Row(f"distance({_t})", "geometric", f"r = {wrap(1, f'distance(A{_s}, B{_s})')};", "vec", width=1,
                    ref=quiet(lambda X, a=a_, b=b_: stack([ref_length([p - q for p, q in zip(a(X), b(X))])])),
                    # the witness is the float64 length of the difference the formula takes (a - b, rounded once per component)
                    witness=witness_relative(lambda X, a=a_, b=b_: [np.sqrt(dot_(*[[(p.astype(F) - q.astype(F)).astype(np.float64) for p, q in zip(a(X), b(X))]]*2))],
                                             (gamma(_n)/2 + U)*1.001, _slots("AB", _n))),
                     Row(f"normalize({_t})", "geometric", f"r = {wrap(_n, f'normalize(A{_s})')};", "vec", width=_n,
                    ref=quiet(lambda X, a=a_: stack([p/ref_length(a(X)) for p in a(X)])),
                    witness=witness_relative(lambda X, a=a_: [p/np.sqrt(dot_(a(X, d=np.float64), a(X, d=np.float64))) for p in a(X, d=np.float64)],
                                             (gamma(_n)/2 + 2*U)*1.001, _slots("A", _n)),
                    note="a/length(a): normalize(0) is NaN")]
    ROWS.extend(_vector_forms if _n > 1 else [])
    ROWS.append(Row(f"reflect({_t})", "geometric", f"r = {wrap(_n, f'reflect(A{_s}, B{_s})')};", "vec", width=_n,
                    ref=quiet(lambda X, a=a_, b=b_: stack([i - (F(2.0)*dot_(b(X), a(X)))*n for i, n in zip(a(X), b(X))])),
                    # dot: N roundings; 2* is exact; *n and the subtraction: N + 2
                    witness=witness_terms(lambda X, sub, a=a_, b=b_: [sub(i, (2.0*dot_(b(X, d=np.float64), a(X, d=np.float64)))*n)
                                                                      for i, n in zip(a(X, d=np.float64), b(X, d=np.float64))], _n + 2, _slots("AB", _n))))
    ROWS.append(Row(f"faceforward({_t})", "geometric", f"r = {wrap(_n, f'faceforward(A{_s}, B{_s}, C{_s})')};", "vec", width=_n,
                    ref=quiet(lambda X, a=a_, b=b_, c=c_: stack([np.where(dot_(c(X), b(X)) < 0, n, -n) for n in a(X)]))))
    ROWS.append(Row(f"refract({_t})", "geometric", f"r = {wrap(_n, f'refract(A{_s}, B{_s}, D.x)')};", "vec", width=_n,
                    ref=quiet(lambda X, a=a_, b=b_: stack(ref_refract(a(X), b(X), part(X, "D", 1)[:, 0])[0])),
                    witness=witness_refract(_n),
                    note="k < 0 (total internal reflection): the zero vector; a NaN k falls through to the formula"))
ROWS.append(Row("cross(vec3)", "geometric", f"r = {wrap(3, 'cross(A.xyz, B.xyz)')};", "vec", width=3,
                ref=quiet(lambda X: stack(cross_(comps(X, "A", 3), comps(X, "B", 3)))),
                witness=witness_terms(lambda X, sub: cross_(comps(X, "A", 3, np.float64), comps(X, "B", 3, np.float64), sub), 2, _slots("AB", 3))))

# ---- operators and constructors of float vectors (§5.4.2, §5.9) -------------------------------------------------------------------
ARITHMETIC = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide}
for _n in (2, 3, 4):
    _t, _s = VEC[_n], SW[_n]
    for _op, _f in ARITHMETIC.items():
        pa, pb, bx = (lambda X, n=_n: part(X, "A", n)), (lambda X, n=_n: part(X, "B", n)), (lambda X: part(X, "B", 1))
        for _name, _body, _ref in ((f"{_t} {_op} {_t}", f"r = {wrap(_n, f'A{_s} {_op} B{_s}')};", lambda X, f=_f, pa=pa, pb=pb: f(pa(X), pb(X))),
                                   (f"{_t} {_op} float", f"r = {wrap(_n, f'A{_s} {_op} B.x')};", lambda X, f=_f, pa=pa, bx=bx: f(pa(X), bx(X))),
                                   (f"float {_op} {_t}", f"r = {wrap(_n, f'B.x {_op} A{_s}')};", lambda X, f=_f, pa=pa, bx=bx: f(bx(X), pa(X))),
                                   (f"{_t} {_op}= {_t}", f"{_t} q = A{_s}; q {_op}= B{_s}; r = {wrap(_n, 'q')};", lambda X, f=_f, pa=pa, pb=pb: f(pa(X), pb(X))),
                                   (f"{_t} {_op}= float", f"{_t} q = A{_s}; q {_op}= B.x; r = {wrap(_n, 'q')};", lambda X, f=_f, pa=pa, bx=bx: f(pa(X), bx(X)))):
            ROWS.append(Row(_name, "geometric", _body, "vec", ref=quiet(_ref), width=_n))
    ROWS.append(Row(f"-{_t}", "geometric", f"r = {wrap(_n, f'-{_t}(A{_s})')};", "vec", ref=lambda X, n=_n: -part(X, "A", n), width=_n))
    ROWS.append(Row(f"+{_t}", "geometric", f"r = {wrap(_n, f'+{_t}(A{_s})')};", "vec", ref=lambda X, n=_n: part(X, "A", n), width=_n))
    # == and !=: against another vector, and against a copy whose .x is B.x (every pair of specials meets there)
    ROWS.append(Row(f"{_t} == {_t}", "geometric", f"{_t} a = A{_s}; {_t} e = a; e.x = B.x; r = vec4(a == {_t}(B{_s}) ? 1.0 : 0.0, a != {_t}(B{_s}) ? 1.0 : 0.0, a == e ? 1.0 : 0.0, a != e ? 1.0 : 0.0);", "vec",
                    ref=quiet(lambda X, n=_n: np.stack([(part(X, "A", n) == part(X, "B", n)).all(1), ~(part(X, "A", n) == part(X, "B", n)).all(1),
                                                        (part(X, "A", n)[:, 1:] == part(X, "A", n)[:, 1:]).all(1) & (X[:, 0] == X[:, 4]),
                                                        ~((part(X, "A", n)[:, 1:] == part(X, "A", n)[:, 1:]).all(1) & (X[:, 0] == X[:, 4]))], 1).astype(F))))
    ROWS.append(Row(f"{_t}(float)", "geometric", f"r = {wrap(_n, f'{_t}(A.y)')};", "vec", ref=lambda X, n=_n: np.repeat(X[:, 1:2], n, 1), width=_n))
_pick16 = lambda *slots: (lambda X: X[:, list(slots)])                                             # noqa: E731
for _name, _body, _slots_ in (("vec3(vec2, float)", "vec4(vec3(A.zw, B.x), 0.0)", (2, 3, 4)), ("vec3(float, vec2)", "vec4(vec3(B.x, A.zw), 0.0)", (4, 2, 3)),
                              ("vec4(vec3, float)", "vec4(A.yzw, B.x)", (1, 2, 3, 4)), ("vec4(float, vec3)", "vec4(B.x, A.yzw)", (4, 1, 2, 3)),
                              ("vec4(vec2, vec2)", "vec4(A.zw, B.xy)", (2, 3, 4, 5)), ("vec4(vec2, float, float)", "vec4(A.zw, B.x, C.y)", (2, 3, 4, 9)),
                              ("vec4(float, vec2, float)", "vec4(B.x, A.zw, C.y)", (4, 2, 3, 9)), ("vec4(float, float, vec2)", "vec4(B.x, C.y, A.zw)", (4, 9, 2, 3)),
                              ("vec2(vec3), vec2(vec4)", "vec4(vec2(B.yzw), vec2(A.wzyx))", (5, 6, 3, 2)), ("vec3(vec4)", "vec4(vec3(A.wzyx), 0.0)", (3, 2, 1))):
    ROWS.append(Row(_name, "geometric", f"r = {_body};", "vec", ref=_pick16(*_slots_), width=len(_slots_)))

# ---- relational functions on float vectors ------------------------------------------------------------------------------------
RELATIONS = {"lessThan": np.less, "lessThanEqual": np.less_equal, "greaterThan": np.greater, "greaterThanEqual": np.greater_equal,
             "equal": np.equal, "notEqual": np.not_equal}
for _n in (2, 3, 4):
    _t, _s = VEC[_n], SW[_n]
    for _name, _op in RELATIONS.items():
        ROWS.append(Row(f"{_name}({_t})", "geometric", f"r = {wrap(_n, f'{_t}({_name}(A{_s}, B{_s}))')};", "vec", width=_n,
                        ref=quiet(lambda X, n=_n, op=_op: op(part(X, "A", n), part(X, "B", n)).astype(F))))
    _p, _q = f"lessThan(A{_s}, B{_s})", f"lessThan(C{_s}, D{_s})"
    lt = lambda X, p, q, n=_n: part(X, p, n) < part(X, q, n)                                       # noqa: E731
    ROWS.append(Row(f"equal(b{_t})", "geometric", f"r = {wrap(_n, f'{_t}(equal({_p}, {_q}))')};", "vec", width=_n, ref=quiet(lambda X, lt=lt: (lt(X, "A", "B") == lt(X, "C", "D")).astype(F))))
    ROWS.append(Row(f"notEqual(b{_t})", "geometric", f"r = {wrap(_n, f'{_t}(notEqual({_p}, {_q}))')};", "vec", width=_n, ref=quiet(lambda X, lt=lt: (lt(X, "A", "B") != lt(X, "C", "D")).astype(F))))
    ROWS.append(Row(f"not(b{_t})", "geometric", f"r = {wrap(_n, f'{_t}(not({_p}))')};", "vec", width=_n, ref=quiet(lambda X, lt=lt: (~lt(X, "A", "B")).astype(F))))
    ROWS.append(Row(f"any, all(b{_t})", "geometric", f"r = vec4(any({_p}) ? 1.0 : 0.0, all({_p}) ? 1.0 : 0.0, any({_q}) ? 1.0 : 0.0, all({_q}) ? 1.0 : 0.0);", "vec",
                    ref=quiet(lambda X, lt=lt: np.stack([lt(X, "A", "B").any(1), lt(X, "A", "B").all(1), lt(X, "C", "D").any(1), lt(X, "C", "D").all(1)], 1).astype(F))))
    # conversions and bit casts of float vectors; integer results leave as words
    ROWS.append(Row(f"i{_t}({_t})", "geometric", f"R = {wrap_words(_n, f'u{_t}(i{_t}(A{_s}))')};", "vec", kind="words", width=_n,
                    ref=lambda X, n=_n: M.ref_to_int(part(X, "A", n)).astype(np.int64) & MASK32))
    ROWS.append(Row(f"u{_t}({_t})", "geometric", f"R = {wrap_words(_n, f'u{_t}(A{_s})')};", "vec", kind="words", width=_n,
                    ref=lambda X, n=_n: M.ref_to_uint(part(X, "A", n)).astype(np.int64)))
    ROWS.append(Row(f"b{_t}({_t})", "geometric", f"r = {wrap(_n, f'{_t}(b{_t}(A{_s}))')};", "vec", width=_n, ref=quiet(lambda X, n=_n: (part(X, "A", n) != 0).astype(F))))
    ROWS.append(Row(f"floatBitsToInt({_t})", "geometric", f"R = {wrap_words(_n, f'u{_t}(floatBitsToInt(A{_s}))')};", "vec", kind="words", width=_n,
                    ref=lambda X, n=_n: M.bits(part(X, "A", n)).astype(np.int64)))
    ROWS.append(Row(f"floatBitsToUint({_t})", "geometric", f"R = {wrap_words(_n, f'floatBitsToUint(A{_s})')};", "vec", kind="words", width=_n,
                    ref=lambda X, n=_n: M.bits(part(X, "A", n)).astype(np.int64)))
    _plus_one = lambda X, n=_n: ((M.bits(part(X, "A", n)).astype(np.int64) + 1) & MASK32).astype(np.uint32).view(F)      # noqa: E731
    ROWS.append(Row(f"intBitsToFloat(i{_t})", "geometric", f"r = {wrap(_n, f'intBitsToFloat(floatBitsToInt(A{_s}) + 1)')};", "vec", width=_n, ref=_plus_one))
    ROWS.append(Row(f"uintBitsToFloat(u{_t})", "geometric", f"r = {wrap(_n, f'uintBitsToFloat(floatBitsToUint(A{_s}) + 1u)')};", "vec", width=_n, ref=_plus_one))


# ---- matrices ---------------------------------------------------------------------------------------------------------------------
# mN, nN: two matrices, vN a vector, s a scalar, cut from the sixteen floats of a point (MATRIX_SLOTS); m[j][i] is column j, row i
MATRIX_SLOTS = {2: (list(range(0, 4)), list(range(4, 8)), [8, 9], 15),
                3: (list(range(0, 9)), list(range(7, 16)), [9, 10, 11], 15),
                4: (list(range(0, 16)), [15, 14, 13, 12, 9, 8, 11, 10, 6, 7, 4, 5, 1, 2, 3, 0], [12, 13, 14, 15], 5)}
_LETTER = [f"{'ABCD'[k//4]}.{'xyzw'[k % 4]}" for k in range(16)]
MATRIX_PREAMBLE = "\n".join(
    f"    mat{n} m{n} = mat{n}({', '.join(_LETTER[k] for k in MATRIX_SLOTS[n][0])}); mat{n} n{n} = mat{n}({', '.join(_LETTER[k] for k in MATRIX_SLOTS[n][1])}); "
    f"vec{n} v{n} = vec{n}({', '.join(_LETTER[k] for k in MATRIX_SLOTS[n][2])}); float s{n} = {_LETTER[MATRIX_SLOTS[n][3]]};" for n in (2, 3, 4))


def mat(X, n, which, dtype=F):
    slots = MATRIX_SLOTS[n][which]
    return [[X[:, slots[j*n + i]].astype(dtype) for i in range(n)] for j in range(n)]


def vec_of(X, n, dtype=F):
    return [X[:, k].astype(dtype) for k in MATRIX_SLOTS[n][2]]


def scalar_of(X, n, dtype=F):
    return X[:, MATRIX_SLOTS[n][3]].astype(dtype)


def flat(m):
    """[[column 0 …] …] -> (points, N*N), column after column"""
    return stack([e for column in m for e in column])


def mv(m, v):
    n = len(v)
    out = []
    for i in range(n):
        s = m[0][i]*v[0]
        for j in range(1, n):
            s = s + m[j][i]*v[j]
        out.append(s)
    return out


def vm(v, m):
    return [dot_(v, column) for column in m]


def mm(a, b):
    return [mv(a, column) for column in b]


def det2(m, sub=minus):
    return sub(m[0][0]*m[1][1], m[1][0]*m[0][1])


def det3(m, sub=minus):
    return plus(sub(m[0][0]*sub(m[1][1]*m[2][2], m[2][1]*m[1][2]), m[1][0]*sub(m[0][1]*m[2][2], m[2][1]*m[0][2])), m[2][0]*sub(m[0][1]*m[1][2], m[1][1]*m[0][2]))


def minor3(m, skip_column, skip_row, sub=minus):
    v = [m[j][i] for j in range(4) if j != skip_column for i in range(4) if i != skip_row]
    return plus(sub(v[0]*sub(v[4]*v[8], v[7]*v[5]), v[3]*sub(v[1]*v[8], v[7]*v[2])), v[6]*sub(v[1]*v[5], v[4]*v[2]))


def det4(m, sub=minus):
    d = np.zeros_like(m[0][0])
    for j in range(4):
        t = m[j][0]*minor3(m, j, 0, sub)
        d = sub(d, t) if j & 1 else d + t
    return d


def determinant(m, sub=minus):
    return {2: det2, 3: det3, 4: det4}[len(m)](m, sub)


def inverse(m):
    n = len(m)
    if n == 2:
        d = det2(m)
        return [[m[1][1]/d, -m[0][1]/d], [-m[1][0]/d, m[0][0]/d]]
    if n == 3:
        a, b, c = m
        rows = [cross_(b, c), cross_(c, a), cross_(a, b)]
        d = dot_(a, rows[0])
        return [[rows[i][j]/d for i in range(3)] for j in range(3)]
    d = det4(m)
    out = [[None]*4 for _ in range(4)]
    for j in range(4):
        for i in range(4):
            c = minor3(m, j, i)
            out[i][j] = (-c if (i + j) & 1 else c)/d
    return out


def resized(m, n):
    size = len(m)
    one, zero = np.ones_like(m[0][0]), np.zeros_like(m[0][0])
    return [[m[j][i] if (i < size and j < size) else (one if i == j else zero) for i in range(n)] for j in range(n)]


def each(f, *ms):
    n = len(ms[0])
    return [[f(*[m[j][i] for m in ms]) for i in range(n)] for j in range(n)]


# the inverse property: max |inverse(m)*m - I|, the product taken in float64, over the matrices of condition number <= 100. Measured on
# the numpy float32 restatement alone; the bound is the next power of two above it
INVERSE_RESIDUAL = {2: (2.0**-18, 2.682e-06), 3: (2.0**-17, 6.622e-06), 4: (2.0**-16, 8.321e-06)}      # {N: (bound, measured on the restatement)}


def inverse_residual(X, got, n) -> np.ndarray:
    m = mat(X, n, 0, np.float64)
    inv = [[got[:, j*n + i].astype(np.float64) for i in range(n)] for j in range(n)]
    with np.errstate(all="ignore"):
        product = mm(inv, m)
        return np.max(np.abs(flat(product) - np.eye(n).reshape(-1)), axis=1)


def matrix_rows(n: int) -> None:
    # (one call per size: the references close over n)
    t, m, o, v, s = f"mat{n}", f"m{n}", f"n{n}", f"v{n}", f"s{n}"
    inputs, kind = f"mat{n}", f"mat{n}"
    slots_m, slots_o, slots_v, slot_s = MATRIX_SLOTS[n]
    M0 = lambda X, n=n, d=F: mat(X, n, 0, d)                                               # noqa: E731
    M1 = lambda X, n=n, d=F: mat(X, n, 1, d)                                               # noqa: E731
    V = lambda X, n=n, d=F: vec_of(X, n, d)                                                # noqa: E731
    S = lambda X, n=n, d=F: scalar_of(X, n, d)                                             # noqa: E731

    def add(name, body, ref, width=n*n, kind=kind, witness=None, note=""):
        ROWS.append(Row(f"{t}: {name}", "matrix", body, inputs, ref=quiet(ref), width=width, kind=kind, witness=witness, note=note))

    add("from N*N scalars", f"{t} R = {m};", lambda X: flat(M0(X)))
    add("from a scalar", f"{t} R = {t}({s});", lambda X: flat(each(lambda e: e, [[S(X) if i == j else np.zeros_like(S(X)) for i in range(n)] for j in range(n)])))
    add("from columns", f"{t} R = {t}({', '.join(f'{o}[{(j + 1) % n}]' for j in range(n))});", lambda X: flat([M1(X)[(j + 1) % n] for j in range(n)]))
    for other in (2, 3, 4):
        if other != n:
            add(f"from mat{other}", f"{t} R = {t}(m{other});", lambda X, other=other: flat(resized(mat(X, other, 0), n)))
    add("m*v", f"r = {wrap(n, f'{m}*{v}')};", lambda X: stack(mv(M0(X), V(X))), width=n, kind="vec",
        witness=witness_terms(lambda X, sub: mv(M0(X, d=np.float64), V(X, d=np.float64)), n, slots_m + slots_v))
    add("v*m", f"r = {wrap(n, f'{v}*{m}')};", lambda X: stack(vm(V(X), M0(X))), width=n, kind="vec",
        witness=witness_terms(lambda X, sub: vm(V(X, d=np.float64), M0(X, d=np.float64)), n, slots_m + slots_v))
    add("m*m", f"{t} R = {m}*{o};", lambda X: flat(mm(M0(X), M1(X))),
        witness=witness_terms(lambda X, sub: [e for c in mm(M0(X, d=np.float64), M1(X, d=np.float64)) for e in c], n, slots_m + slots_o))
    for op, f in (("*", np.multiply), ("/", np.divide), ("+", np.add), ("-", np.subtract)):
        add(f"m {op} s", f"{t} R = {m} {op} {s};", lambda X, f=f: flat(each(lambda e: f(e, S(X)), M0(X))))
        add(f"s {op} m", f"{t} R = {s} {op} {m};", lambda X, f=f: flat(each(lambda e: f(S(X), e), M0(X))))
        add(f"m {op}= s", f"{t} R = {m}; R {op}= {s};", lambda X, f=f: flat(each(lambda e: f(e, S(X)), M0(X))))
    for op, f in (("+", np.add), ("-", np.subtract), ("/", np.divide)):
        add(f"m {op} m", f"{t} R = {m} {op} {o};", lambda X, f=f: flat(each(f, M0(X), M1(X))))
        add(f"m {op}= m", f"{t} R = {m}; R {op}= {o};", lambda X, f=f: flat(each(f, M0(X), M1(X))))
    add("m *= m", f"{t} R = {m}; R *= {o};", lambda X: flat(mm(M0(X), M1(X))))
    add("-m", f"{t} R = -{m};", lambda X: flat(each(np.negative, M0(X))))
    add("== and !=", f"{t} c = {m}; {t} e = {m}; e[{n - 1}][0] = {s}; r = vec4({m} == c ? 1.0 : 0.0, {m} != c ? 1.0 : 0.0, {m} == e ? 1.0 : 0.0, {m} != e ? 1.0 : 0.0);",
        lambda X: np.stack([(flat(M0(X)) == flat(M0(X))).all(1), ~(flat(M0(X)) == flat(M0(X))).all(1),
                            (flat(M0(X)) == flat(M0(X))).all(1) & (M0(X)[n - 1][0] == S(X)),
                            ~((flat(M0(X)) == flat(M0(X))).all(1) & (M0(X)[n - 1][0] == S(X)))], 1).astype(F), width=4, kind="vec",
        note="component-wise ==: a NaN component makes a matrix unequal to its own copy")
    add("matrixCompMult", f"{t} R = matrixCompMult({m}, {o});", lambda X: flat(each(np.multiply, M0(X), M1(X))))
    add("transpose", f"{t} R = transpose({m});", lambda X: flat([[M0(X)[i][j] for i in range(n)] for j in range(n)]))
    add("outerProduct", f"{t} R = outerProduct({v}, {o}[0]);", lambda X: flat([[c*M1(X)[0][j] for c in V(X)] for j in range(n)]))
    add("v.swizzle *= m", f"vec4 q = vec4({v}{', 7.0' if n == 3 else ', 7.0, 9.0' if n == 2 else ''}); q{SW[n] or '.xyzw'} *= {m}; r = q;",
        lambda X: np.concatenate([stack(vm(V(X), M0(X))), np.tile(np.array([7.0, 9.0][:4 - n], F), (len(X), 1))], 1), width=4, kind="vec")
    # determinant: the longest path rounds 2 / 5 / 10 times (products, the inner and outer differences, the accumulation)
    add("determinant", f"r = {wrap(1, f'determinant({m})')};", lambda X: stack([determinant(M0(X))]), width=1, kind="vec",
        witness=witness_terms(lambda X, sub: [determinant(M0(X, d=np.float64), sub)], {2: 2, 3: 5, 4: 10}[n], slots_m))
    add("inverse", f"{t} R = inverse({m});", lambda X: flat(inverse(M0(X))),
        note="cofactors over the determinant: a singular matrix gives inf/NaN, held by the restatement only")


for _n in (2, 3, 4):
    matrix_rows(_n)


# ---- integers -------------------------------------------------------------------------------------------------------------------
INTEGER_PREAMBLE = """    uvec4 ua = uvec4(word(A.x, A.y), word(A.z, A.w), word(B.x, B.y), word(B.z, B.w));
    uvec4 ub = uvec4(word(C.x, C.y), word(C.z, C.w), word(D.x, D.y), word(D.z, D.w));
    ivec4 ia = ivec4(ua); ivec4 ib = ivec4(ub);"""


def signed(w):
    return ((np.asarray(w, np.int64) & MASK32) ^ (1 << 31)) - (1 << 31)


def _div(a, b, sign):
    if not sign:
        return a//b
    q = np.abs(a)//np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


INT_OPS = {
    "+": lambda a, b, sign: a + b,
    "-": lambda a, b, sign: a - b,
    "*": lambda a, b, sign: ((a & MASK32).astype(np.uint64)*(b & MASK32).astype(np.uint64)).astype(np.int64),      # wraps mod 2^64: the low word is right
    "/": _div,
    "%": lambda a, b, sign: a - b*_div(a, b, sign),
    "&": lambda a, b, sign: a & b,
    "|": lambda a, b, sign: a | b,
    "^": lambda a, b, sign: a ^ b,
    "<<": lambda a, b, sign: (a & MASK32) << b,
    ">>": lambda a, b, sign: a >> b,
}
INT_INPUTS = {"/": "div", "%": "div", "<<": "shift", ">>": "shift"}


def _int_min(a, b):
    return np.where(b < a, b, a)


def _int_max(a, b):
    return np.where(a < b, b, a)


def _int_clamp(x, lo, hi):
    v = np.where(x < lo, lo, x)
    return np.where(v > hi, hi, v)


def integer_rows(scalar: str, prefix: str, sign: bool, n: int) -> None:
    # (one call per type and size: the references close over them)
    view = signed if sign else (lambda w: np.asarray(w, np.int64) & MASK32)
    t, sw = (scalar if n == 1 else f"{prefix}vec{n}"), SW[n]
    a, b = f"{prefix}a{sw}", f"{prefix}b{sw}"
    unsigned = "uint" if n == 1 else f"uvec{n}"
    out = (lambda e, n=n, convert=sign, unsigned=unsigned: f"R = {wrap_words(n, f'{unsigned}({e})' if convert else e)};")
    A_ = lambda W, n=n: view(W[:, 0:n])                                                    # noqa: E731
    B_ = lambda W, n=n: view(W[:, 4:4 + n])                                                # noqa: E731
    AX = lambda W: view(W[:, 0:1])                                                         # noqa: E731
    BX = lambda W: view(W[:, 4:5])                                                         # noqa: E731

    def add(name, body, ref, inputs="int", kind="words", width=n, note="", fragment="integer"):
        ROWS.append(Row(f"{t}: {name}", fragment, body, inputs, ref=quiet(lambda W, ref=ref: ref(W) & MASK32 if kind == "words" else ref(W)),
                        width=width, kind=kind, note=note))

    for op, f in INT_OPS.items():
        inputs = INT_INPUTS.get(op, "int")
        add(f"a {op} b", out(f"{a} {op} {b}"), lambda W, f=f: f(A_(W), B_(W), sign), inputs)
        add(f"a {op}= b", f"{t} q = {a}; q {op}= {b}; " + out("q"), lambda W, f=f: f(A_(W), B_(W), sign), inputs)
        if n > 1:
            add(f"a {op} scalar", out(f"{a} {op} {prefix}b.x"), lambda W, f=f: f(A_(W), BX(W), sign), inputs)
            add(f"scalar {op} b", out(f"{prefix}a.x {op} {b}"), lambda W, f=f: f(AX(W), B_(W), sign), inputs)
            add(f"a {op}= scalar", f"{t} q = {a}; q {op}= {prefix}b.x; " + out("q"), lambda W, f=f: f(A_(W), BX(W), sign), inputs)
    add("-a", out(f"-{a}"), lambda W: -A_(W), note="wraps: -INT_MIN is INT_MIN")
    add("~a", out(f"~{a}"), lambda W: ~A_(W))
    hi = f"{prefix}b.{'wzyx'[:n]}"
    HI = lambda W, n=n: view(W[:, [7, 6, 5, 4][:n]])                                       # noqa: E731
    # the scalar uint forms existed before this table, comparing as int: a probe of their own, which compiles without the
    # vector forms and shows the wrong values
    own = "uint" if (n == 1 and not sign) else "integer"
    add("min(a, b)", out(f"min({a}, {b})"), lambda W: _int_min(A_(W), B_(W)), fragment=own)
    add("max(a, b)", out(f"max({a}, {b})"), lambda W: _int_max(A_(W), B_(W)), fragment=own)
    add("clamp(a, b, c)", out(f"clamp({a}, {b}, {hi})"), lambda W: _int_clamp(A_(W), B_(W), HI(W)), note="lo > hi is what the formula gives: min(max(x, lo), hi)", fragment=own)
    if n > 1:
        add("min(a, scalar)", out(f"min({a}, {prefix}b.x)"), lambda W: _int_min(A_(W), BX(W)))
        add("max(a, scalar)", out(f"max({a}, {prefix}b.x)"), lambda W: _int_max(A_(W), BX(W)))
        add("clamp(a, scalar, scalar)", out(f"clamp({a}, {prefix}b.x, {prefix}b.y)"), lambda W: _int_clamp(A_(W), BX(W), view(W[:, 5:6])))
    if sign:
        add("abs(a)", out(f"abs({a})"), lambda W: np.abs(A_(W)), note="abs(INT_MIN) stays INT_MIN (-fwrapv)")
        add("sign(a)", out(f"sign({a})"), lambda W: np.sign(A_(W)))
    if n > 1:
        other = ("u" if sign else "i") + f"vec{n}"
        add(f"{other}(a)", out(f"{other}({a})", convert=not sign), lambda W: A_(W))
        add(f"vec{n}(a)", f"r = {wrap(n, f'vec{n}({a})')};", lambda W: A_(W).astype(F), kind="vec", note="int -> float rounds to nearest even")
        add(f"bvec{n}(a)", f"r = {wrap(n, f'vec{n}(bvec{n}({a}))')};", lambda W: (A_(W) != 0).astype(F), kind="vec")
        add(f"from bvec{n}", out(f"{t}(lessThan({a}, {b}))"), lambda W: (A_(W) < B_(W)).astype(np.int64))
        same = lambda W: (A_(W) == B_(W)).all(1)                                               # noqa: E731
        head = lambda W: W[:, 0] == W[:, 4]                                                    # noqa: E731
        add("a == b, a != b", f"{t} e = {a}; e.x = {prefix}b.x; r = vec4({a} == {b} ? 1.0 : 0.0, {a} != {b} ? 1.0 : 0.0, {a} == e ? 1.0 : 0.0, {a} != e ? 1.0 : 0.0);",
            lambda W: np.stack([same(W), ~same(W), head(W), ~head(W)], 1).astype(F), kind="vec", width=4)
        add("from a scalar", out(f"{t}({prefix}b.y)"), lambda W: np.repeat(view(W[:, 5:6]), n, 1))
        for name, op in RELATIONS.items():
            add(f"{name}(a, b)", f"r = {wrap(n, f'vec{n}({name}({a}, {b}))')};", lambda W, op=op: op(A_(W), B_(W)).astype(F), kind="vec")


for _scalar, _prefix, _sign in (("int", "i", True), ("uint", "u", False)):
    for _n in (1, 2, 3, 4):
        integer_rows(_scalar, _prefix, _sign, _n)
for _p in "iu":
    for _name, _body, _slots_ in ((f"{_p}vec3({_p}vec2, scalar)", f"uvec4(uvec3({_p}vec3({_p}a.zw, {_p}b.x)), 0u)", (2, 3, 4)),
                                  (f"{_p}vec3(scalar, {_p}vec2)", f"uvec4(uvec3({_p}vec3({_p}b.x, {_p}a.zw)), 0u)", (4, 2, 3)),
                                  (f"{_p}vec4({_p}vec3, scalar)", f"uvec4({_p}vec4({_p}a.yzw, {_p}b.x))", (1, 2, 3, 4)),
                                  (f"{_p}vec4({_p}vec2, {_p}vec2)", f"uvec4({_p}vec4({_p}a.zw, {_p}b.xy))", (2, 3, 4, 5)),
                                  (f"{_p}vec4({_p}vec2, scalar, scalar)", f"uvec4({_p}vec4({_p}a.zw, {_p}b.x, {_p}b.w))", (2, 3, 4, 7))):
        ROWS.append(Row(_name, "integer", f"R = {_body};", "int", ref=lambda W, k=_slots_: W[:, list(k)] & MASK32, kind="words", width=len(_slots_)))
ROWS.append(Row("words in, words out", "integer", "R = uvec4(ua.x, ub.y, ia.z, ib.w);", "int", ref=lambda W: W[:, [0, 5, 2, 7]] & MASK32, kind="words"))


# ---- swizzles (selection does not depend on the data: 4 x 4 points) -----------------------------------------------------------------
NAMES = "xyzw"
SWIZZLE_SIZE = (4, 4)


def _pick(letters: str, source: int = 4):
    index = [NAMES.index(c) for c in letters]
    return lambda X: part(X, "A", source)[:, index]


def swizzle_rows() -> None:
    def add(name, body, ref, width=4):
        fragment = "swizzle writes" if ("=" in name or name == "vec4.bgr = t") else "swizzle"
        ROWS.append(Row(name, fragment, body, "swizzle", ref=quiet(ref), width=width, size=SWIZZLE_SIZE))

    for letters in map("".join, itertools.product(NAMES, repeat=4)):                               # all 256 reads of four components
        add(f"vec4.{letters}", f"r = A.{letters};", _pick(letters))
    for source in (2, 3, 4):
        for count in (2, 3):
            for letters in map("".join, itertools.product(NAMES[:source], repeat=count)):
                add(f"vec{source}.{letters}", f"vec{source} q = vec{source}(A{SW[source]}); r = {wrap(count, f'q.{letters}')};", _pick(letters), count)
    for family, make, back in (("vec4", "A", "q"), ("ivec4", "ivec4(A)", "vec4(q)"), ("uvec4", "uvec4(A)", "vec4(q)")):
        for count in (2, 3, 4):
            for letters in map("".join, itertools.permutations(NAMES, count)):                         # every permutation write
                source = {"vec4": f"B{SW[count]}", "ivec4": f"ivec{count}(B{SW[count]})", "uvec4": f"uvec{count}(B{SW[count]})"}[family]

                def ref(X, letters=letters):
                    out = part(X, "A").copy()
                    for k, c in enumerate(letters):
                        out[:, NAMES.index(c)] = part(X, "B")[:, k]
                    return out
                add(f"{family}.{letters} = t", f"{family} q = {make}; q.{letters} = {source}; r = {back};", ref)
    for other, letters in (("rgba", "wzyx"), ("stpq", "yxwz"), ("rgba", "xxzz"), ("stpq", "wwww")):
        named = "".join(other[NAMES.index(c)] for c in letters)
        add(f"vec4.{named}", f"r = A.{named};", _pick(letters))
    add("vec4.bgr = t", "vec4 q = A; q.bgr = B.xyz; r = q;", lambda X: np.stack([part(X, "B")[:, 2], part(X, "B")[:, 1], part(X, "B")[:, 0], part(X, "A")[:, 3]], 1))
    add("vec4.ts = t", "vec4 q = A; q.ts = B.xy; r = q;", lambda X: np.stack([part(X, "B")[:, 1], part(X, "B")[:, 0], part(X, "A")[:, 2], part(X, "A")[:, 3]], 1))
    # aliasing and compound writes: the right-hand side is read before anything is written
    add("v.xy = v.yx", "vec4 q = A; q.xy = q.yx; r = q;", _pick("yxzw"))
    add("v.yzw = v.xyz", "vec4 q = A; q.yzw = q.xyz; r = q;", _pick("xxyz"))
    add("v.zw += v.xy", "vec4 q = A; q.zw += q.xy; r = q;", lambda X: np.stack([part(X, "A")[:, 0], part(X, "A")[:, 1], part(X, "A")[:, 2] + part(X, "A")[:, 0], part(X, "A")[:, 3] + part(X, "A")[:, 1]], 1))
    add("v.wzyx *= 2.0", "vec4 q = A; q.wzyx *= 2.0; r = q;", lambda X: part(X, "A")*F(2.0))
    add("v.xz -= v.zx", "vec4 q = A; q.xz -= q.zx; r = q;", lambda X: np.stack([part(X, "A")[:, 0] - part(X, "A")[:, 2], part(X, "A")[:, 1], part(X, "A")[:, 2] - part(X, "A")[:, 0], part(X, "A")[:, 3]], 1))
    add("i.yx <<= 1", "ivec4 q = ivec4(A); q.yx <<= 1; r = vec4(q);", lambda X: part(X, "A")*np.array([2, 2, 1, 1], F))
    add("u.zw = u.wz", "uvec4 q = uvec4(A); q.zw = q.wz; r = vec4(q);", _pick("xywz"))


swizzle_rows()


# ---- the prelude (include/shaderflow.glsl, complex.glsl as restated in jit_runtime.hpp) -------------------------------------------
def col(X, k):
    return X[:, k]


def ref_smoothlerp(a, b, d):
    t = M.ref_clamp((a - b)/d + F(0.5), F(0.0), F(1.0))
    offset = d*t*(F(1.0) - t)/F(2.0)
    return M.ref_mix(a, b, t) - offset


def ref_triangle_wave(x, period):
    return F(2.0)*np.abs(M.ref_mod(F(2.0)*x/period - F(0.5), F(2.0)) - F(1.0)) - F(1.0)


def ref_sd_line(o, a, b, segment):
    direction, shortest = [q - p for p, q in zip(a, b)], [q - p for p, q in zip(a, o)]
    t = dot_(shortest, direction)/dot_(direction, direction)
    if segment:
        t = M.ref_clamp(t, F(0.0), F(1.0))
    return ref_length([s - d*t for s, d in zip(shortest, direction)])


def ref_rgb2hsv(r, g, b):
    cmax, cmin = M.ref_max(r, M.ref_max(g, b)), M.ref_min(r, M.ref_min(g, b))
    delta = cmax - cmin
    h = np.where(delta == 0, F(0.0), np.where(cmax == r, M.ref_mod((g - b)/delta, F(6.0)), np.where(cmax == g, (b - r)/delta + F(2.0), (r - g)/delta + F(4.0)))).astype(F)
    h = h*(F(np.float32(np.pi))/F(3.0))
    return [h, np.where(cmax == 0, F(0.0), delta/cmax).astype(F), cmax]


def ref_black_key(index):
    key = np.fmod(index.astype(np.int64), 12)                                              # C's %: the dividend's sign
    return np.isin(key, (1, 3, 6, 8, 10))


def prelude_rows() -> None:
    def add(name, body, ref, width=1, **more):
        ROWS.append(Row(name, "prelude", body, "vec", ref=quiet(ref) if ref else None, width=width, **more))

    a, b, c, d = (lambda X, n=3, k=k: [X[:, 4*k + j] for j in range(n)] for k in range(4))
    x = col
    PI32, TAU32 = F(np.float32(np.pi)), F(np.float32(2*np.pi))
    one = lambda v: stack([v])                                                             # noqa: E731
    add("proportion", "r.x = proportion(A.x, A.y, A.z);", lambda X: one((x(X, 1)*x(X, 2))/x(X, 0)))
    add("lerp", "r.x = lerp(A.x, A.y, A.z, A.w, B.x);", lambda X: one(x(X, 1) + (x(X, 4) - x(X, 0))*(x(X, 3) - x(X, 1))/(x(X, 2) - x(X, 0))))
    add("smoothlerp, smin, smax", "r = vec4(smoothlerp(A.x, A.y, A.z), smin(A.x, A.y, A.z), smax(A.x, A.y, A.z), smin(A.x, A.y) + 0.0*smax(A.x, A.y));",
        lambda X: stack([ref_smoothlerp(x(X, 0), x(X, 1), x(X, 2)), ref_smoothlerp(x(X, 0), x(X, 1), x(X, 2)), ref_smoothlerp(x(X, 0), x(X, 1), -x(X, 2)),
                         ref_smoothlerp(x(X, 0), x(X, 1), F(1.0)) + F(0.0)*ref_smoothlerp(x(X, 0), x(X, 1), F(-1.0))]), 4)
    add("smin, smax (two arguments)", "r = vec4(smin(A.x, A.y), smax(A.x, A.y), 0.0, 0.0);",
        lambda X: stack([ref_smoothlerp(x(X, 0), x(X, 1), F(1.0)), ref_smoothlerp(x(X, 0), x(X, 1), F(-1.0))]), 2)
    add("smoothmix", "r.x = smoothmix(A.x, A.y, A.z, A.w, B.x);", lambda X: one(M.ref_mix(x(X, 0), x(X, 1), M.ref_smoothstep(x(X, 2), x(X, 3), x(X, 4)))))
    add("triangle_wave", "r.x = triangle_wave(A.x, A.y);", lambda X: one(ref_triangle_wave(x(X, 0), x(X, 1))))
    add("stuv2gluv, gluv2stuv", "r = vec4(stuv2gluv(A.xy), gluv2stuv(A.zw));",
        lambda X: stack([x(X, 0)*F(2.0) - F(1.0), x(X, 1)*F(2.0) - F(1.0), (x(X, 2) + F(1.0))/F(2.0), (x(X, 3) + F(1.0))/F(2.0)]), 4)
    add("stuv2stxy, stxy2stuv", "r = vec4(stuv2stxy(A.xy, B.xy), stxy2stuv(A.zw, B.zw));", lambda X: stack([x(X, 4)*x(X, 0), x(X, 5)*x(X, 1), x(X, 2)/x(X, 6), x(X, 3)/x(X, 7)]), 4)
    add("agluv_mirrored_repeat", "r = vec4(agluv_mirrored_repeat(A.xy), 0.0, 0.0);", lambda X: stack([ref_triangle_wave(x(X, 0), F(4.0)), ref_triangle_wave(x(X, 1), F(4.0))]), 2)
    add("astuv_oob, agluv_oob", "r = vec4(astuv_oob(A.xy) ? 1.0 : 0.0, agluv_oob(A.xy) ? 1.0 : 0.0, 0.0, 0.0);",
        lambda X: stack([((x(X, 0) < 0) | (x(X, 0) > 1) | (x(X, 1) < 0) | (x(X, 1) > 1)).astype(F), ((x(X, 0) < -1) | (x(X, 0) > 1) | (x(X, 1) < -1) | (x(X, 1) > 1)).astype(F)]), 2)

    def ref_palette(X):
        t = x(X, 15)*F(0.25)
        low = [M.ref_mix(p, q, t*F(4.0)) for p, q in zip(a(X), b(X))]
        middle = [M.ref_mix(p, q, (t - F(0.25))*F(4.0)) for p, q in zip(b(X), c(X))]
        high = [M.ref_mix(p, q, (t - F(0.5))*F(4.0)) for p, q in zip(c(X), d(X))]
        return stack([np.where(t < F(0.25), l, np.where(t < F(0.5), m, h)) for l, m, h in zip(low, middle, high)])
    add("palette", "r = vec4(palette(D.w*0.25, A.xyz, B.xyz, C.xyz, D.xyz), 0.0);", ref_palette, 3)
    add("isBlackKey, isWhiteKey", "r = vec4(isBlackKey(A.x*16.0) ? 1.0 : 0.0, isWhiteKey(A.x*16.0) ? 1.0 : 0.0, isBlackKey(int(A.y*16.0) + 60) ? 1.0 : 0.0, isWhiteKey(int(A.y*16.0) + 60) ? 1.0 : 0.0);",
        lambda X: stack([ref_black_key(M.ref_to_int(x(X, 0)*F(16.0))), ~ref_black_key(M.ref_to_int(x(X, 0)*F(16.0))),
                         ref_black_key(signed(M.ref_to_int(x(X, 1)*F(16.0)).astype(np.int64) + 60)), ~ref_black_key(signed(M.ref_to_int(x(X, 1)*F(16.0)).astype(np.int64) + 60))]).astype(F), 4)
    zero = lambda X: np.zeros(len(X), F)                                                   # noqa: E731
    flat2 = lambda v, X: [v(X, 2)[0], v(X, 2)[1], zero(X)]                                 # noqa: E731
    add("sdLine, sdLineSegment", "r = vec4(sdLine(A.xyz, B.xyz, C.xyz), sdLineSegment(A.xyz, B.xyz, C.xyz), sdLine(A.xy, B.xy, C.xy), sdLineSegment(A.xy, B.xy, C.xy));",
        lambda X: stack([ref_sd_line(a(X), b(X), c(X), False), ref_sd_line(a(X), b(X), c(X), True),
                         ref_sd_line(flat2(a, X), flat2(b, X), flat2(c, X), False), ref_sd_line(flat2(a, X), flat2(b, X), flat2(c, X), True)]), 4)
    add("sdSphere, sdPlane, sdOctahedron", "r = vec4(sdSphere(A.xyz, B.xyz, C.x), sdPlane(A.xyz, B.xyz, C.xyz), sdOctahedron(A.xyz, B.xyz, C.x), 0.0);",
        lambda X: stack([ref_length([q - p for p, q in zip(a(X), b(X))]) - x(X, 8),
                         dot_([p - q for p, q in zip(a(X), b(X))], [n/ref_length(c(X)) for n in c(X)]),
                         F(np.float32(1.7320508075688772))*(np.abs(x(X, 0) - x(X, 4)) + np.abs(x(X, 1) - x(X, 5)) + np.abs(x(X, 2) - x(X, 6)) - x(X, 8))]), 3)

    def ref_sd_box(X):
        e = [np.abs(p - q) - s/F(2.0) for p, q, s in zip(a(X), b(X), c(X))]
        return one(M.ref_min(M.ref_max(e[0], M.ref_max(e[1], e[2])), F(0.0)) + ref_length([M.ref_max(v, F(0.0)) for v in e]))
    add("sdBox", "r.x = sdBox(A.xyz, B.xyz, C.xyz);", ref_sd_box)

    def ref_smooth(X, which):
        p, q, w = x(X, 0), x(X, 1), x(X, 2)
        if which == "union":
            k = M.ref_clamp(F(0.5) + F(0.5)*(q - p)/w, F(0.0), F(1.0))
            return M.ref_mix(q, p, k) - w*k*(F(1.0) - k)
        if which == "subtraction":
            k = M.ref_clamp(F(0.5) - F(0.5)*(q + p)/w, F(0.0), F(1.0))
            return M.ref_mix(q, -p, k) + w*k*(F(1.0) - k)
        k = M.ref_clamp(F(0.5) - F(0.5)*(q - p)/w, F(0.0), F(1.0))
        return M.ref_mix(q, p, k) + w*k*(F(1.0) - k)
    add("sdUnion, sdSubtraction, sdIntersection", "r = vec4(sdUnion(A.x, A.y), sdSubtraction(A.x, A.y), sdIntersection(A.x, A.y), 0.0);",
        lambda X: stack([M.ref_min(x(X, 0), x(X, 1)), M.ref_max(x(X, 1), -x(X, 0)), M.ref_max(x(X, 0), x(X, 1))]), 3)
    add("sdSmoothUnion, …Subtraction, …Intersection", "r = vec4(sdSmoothUnion(A.x, A.y, A.z), sdSmoothSubtraction(A.x, A.y, A.z), sdSmoothIntersection(A.x, A.y, A.z), 0.0);",
        lambda X: stack([ref_smooth(X, "union"), ref_smooth(X, "subtraction"), ref_smooth(X, "intersection")]), 3)
    A4, B4 = (lambda X: [X[:, j] for j in range(4)]), (lambda X: [X[:, 4 + j] for j in range(4)])
    add("blend", "r = blend(A, B);", lambda X: stack([M.ref_mix(p, q, x(X, 7)) for p, q in zip(A4(X), B4(X))]), 4)
    add("alpha_composite", "r = alpha_composite(A, B);", lambda X: stack([p*(F(1.0) - x(X, 7)) + q*x(X, 7) for p, q in zip(A4(X), B4(X))]), 4)
    for n in (2, 3, 4):
        add(f"saturate(vec{n})", f"r = {wrap(n, f'saturate(A{SW[n]}, B.x)')};", lambda X, n=n: stack([M.ref_clamp(X[:, j]*x(X, 4), F(0.0), F(1.0)) for j in range(n)]), n)
    add("zoom", "r = vec4(zoom(A.xy, B.x, C.xy), zoom(A.xy, B.x));",
        lambda X: stack([(x(X, 0) - x(X, 8))*(x(X, 4)*x(X, 4)) + x(X, 8), (x(X, 1) - x(X, 9))*(x(X, 4)*x(X, 4)) + x(X, 9), x(X, 0)*(x(X, 4)*x(X, 4)), x(X, 1)*(x(X, 4)*x(X, 4))]), 4)
    add("rgb2hsv(vec3)", "r = vec4(rgb2hsv(A.xyz), 0.0);", lambda X: stack(ref_rgb2hsv(x(X, 0), x(X, 1), x(X, 2))), 3)
    add("rgb2hsv(vec4), rgb2hsv(r, g, b)", "r = rgb2hsv(A) + 0.0*vec4(rgb2hsv(A.x, A.y, A.z), 0.0);",
        lambda X: stack([h + F(0.0)*h for h in ref_rgb2hsv(x(X, 0), x(X, 1), x(X, 2))] + [x(X, 3) + F(0.0)*F(0.0)]), 4)
    add("cadd, csub", "r = vec4(cadd(A.xy, B.xy), csub(A.xy, B.xy));", lambda X: stack([x(X, 0) + x(X, 4), x(X, 1) + x(X, 5), x(X, 0) - x(X, 4), x(X, 1) - x(X, 5)]), 4)
    add("cmul, cconj", "r = vec4(cmul(A.xy, B.xy), cconj(A.xy));", lambda X: stack([x(X, 0)*x(X, 4) - x(X, 1)*x(X, 5), x(X, 0)*x(X, 5) + x(X, 1)*x(X, 4), x(X, 0), -x(X, 1)]), 4)

    def ref_cdiv(X):
        den = x(X, 4)*x(X, 4) + x(X, 5)*x(X, 5)
        return stack([(x(X, 0)*x(X, 4) + x(X, 1)*x(X, 5))/den, (x(X, 1)*x(X, 4) - x(X, 0)*x(X, 5))/den, ref_length([x(X, 0), x(X, 1)])])
    add("cdiv, cmag", "r = vec4(cdiv(A.xy, B.xy), cmag(A.xy), 0.0);", ref_cdiv, 3)

    # what calls sin / cos / atan / exp: the composition of this probe's own scalar results (bounded in math_cases) with float32 operations
    add("parts: cos, sin, exp, atan", "r = vec4(cos(A.x), sin(A.x), exp(A.x), atan(A.x));", None, 4, note="scalar forms bounded in math_cases: device = host here")
    add("parts: atan(y, x)", "r = vec4(atan(A.x, B.x), atan(-A.x, B.x), 0.0, 0.0);", None, 2, note="scalar forms bounded in math_cases: device = host here")
    one_, two_ = "parts: cos, sin, exp, atan", "parts: atan(y, x)"
    add("rotate2d", "mat2 m = rotate2d(A.x); r = vec4(m[0], m[1]);", lambda X, p: np.stack([p[:, 0], -p[:, 1], p[:, 1], p[:, 0]], 1), 4, uses=(one_,))
    add("polar2rect, ccar", "r = vec4(polar2rect(A.y, A.x), ccar(A.yx));", lambda X, p: np.stack([x(X, 1)*p[:, 0], x(X, 1)*p[:, 1], x(X, 1)*p[:, 0], x(X, 1)*p[:, 1]], 1), 4, uses=(one_,))
    add("cexp", "r = vec4(cexp(A.xx), 0.0, 0.0);", lambda X, p: np.stack([p[:, 2]*p[:, 0], p[:, 2]*p[:, 1]], 1), 2, uses=(one_,))
    add("atan_normalized", "r.x = atan_normalized(A.x);", lambda X, p: one(F(2.0)*p[:, 3]/PI32), 1, uses=(one_,))
    add("atan1, atan1n, cpol", "r = vec4(atan1(vec2(B.x, A.x)), atan1n(vec2(B.x, A.x)), cpol(vec2(B.x, A.x)));",
        lambda X, q: np.stack([q[:, 0], q[:, 0]/PI32, ref_length([x(X, 4), x(X, 0)]), q[:, 0]], 1), 4, uses=(two_,))
    add("atan2, atan2n", "r = vec4(atan2(A.x, B.x), atan2n(A.x, B.x), atan2(vec2(B.x, A.x)), atan2n(vec2(B.x, A.x)));",
        lambda X, q: np.stack([np.where(x(X, 0) < 0, TAU32 - q[:, 1], q[:, 0]), np.where(x(X, 0) < 0, TAU32 - q[:, 1], q[:, 0])/TAU32]*2, 1), 4, uses=(two_,))
    add("parts: cos, sin of B.x", "r = vec4(cos(B.x), sin(B.x), 0.0, 0.0);", None, 2, note="scalar forms bounded in math_cases: device = host here")
    three_ = "parts: cos, sin of B.x"
    add("sphere2rect", "r = vec4(sphere2rect(C.x, A.x, B.x), 0.0);",
        lambda X, p, q: np.stack([x(X, 8)*p[:, 1]*q[:, 0], x(X, 8)*p[:, 1]*q[:, 1], x(X, 8)*p[:, 0]], 1), 3, uses=(one_, three_))

    def ref_rotate3d(X, p):
        v, axis = b(X), c(X)
        along = dot_(axis, v)
        turned = cross_(axis, v)
        return np.stack([M.ref_mix(along*e, w, p[:, 0]) + t*p[:, 1] for e, w, t in zip(axis, v, turned)], 1)
    add("rotate3d", "r = vec4(rotate3d(B.xyz, C.xyz, A.x), 0.0);", ref_rotate3d, 3, uses=(one_,))
    # angle: the quotient restated in float32, then the header's acos of it (ref_acos: the same composition the `acos` row of the
    # component-wise probe is held to on the probe's own results)
    def ref_angle(X):
        out = []
        for n in (2, 3, 4):
            p, q = [X[:, j] for j in range(n)], [X[:, 4 + j] for j in range(n)]
            out.append(ref_acos(dot_(p, q)/(ref_length(p)*ref_length(q))))
        return stack(out)
    add("angle", "r = vec4(angle(A.xy, B.xy), angle(A.xyz, B.xyz), angle(A, B), 0.0);", ref_angle, 3)

    def ref_hsv2rgb(h, s_, v):
        """glsl.hpp hsv2rgb: formula-defined throughout (mod, abs, floor, to_int)"""
        h = M.ref_mod(h, TAU32)
        chroma = v*s_
        second = chroma*(F(1.0) - np.abs(M.ref_mod(h/(PI32/F(3.0)), F(2.0)) - F(1.0)))
        m = v - chroma
        sector = M.ref_to_int(np.floor(F(6.0)*(h/(F(2.0)*PI32))))
        zero_ = np.zeros_like(chroma)
        table = {0: (chroma, second, zero_), 1: (second, chroma, zero_), 2: (zero_, chroma, second), 3: (zero_, second, chroma), 4: (second, zero_, chroma), 5: (chroma, zero_, second)}
        out = []
        for channel in range(3):
            value = zero_
            for which, triple in table.items():
                value = np.where(sector == which, triple[channel], value)
            out.append((value + m).astype(F))
        return out
    add("hsv2rgb(vec3)", "r = vec4(hsv2rgb(A.xyz), 0.0);", lambda X: stack(ref_hsv2rgb(x(X, 0), x(X, 1), x(X, 2))), 3)
    add("hsv2rgb(vec4)", "r = hsv2rgb(A);", lambda X: stack(ref_hsv2rgb(x(X, 0), x(X, 1), x(X, 2)) + [x(X, 3)]), 4)
    add("hsv2rgb(h, s, v)", "r = vec4(hsv2rgb(A.x*2.0, A.y, A.z), 0.0);", lambda X: stack(ref_hsv2rgb(x(X, 0)*F(2.0), x(X, 1), x(X, 2))), 3)
    # the aliases and the macros
    add("smix", "r.x = smix(A.x, A.y, A.z, A.w, B.x);", lambda X: one(M.ref_mix(x(X, 0), x(X, 1), M.ref_smoothstep(x(X, 2), x(X, 3), x(X, 4)))))
    add("s2g, g2s", "r = vec4(s2g(A.xy), g2s(A.zw));", lambda X: stack([x(X, 0)*F(2.0) - F(1.0), x(X, 1)*F(2.0) - F(1.0), (x(X, 2) + F(1.0))/F(2.0), (x(X, 3) + F(1.0))/F(2.0)]), 4)
    magma = [np.array(v, F) for v in ((0.01060815, 0.01808215, 0.10018654), (0.38092887, 0.12061482, 0.32506528), (0.79650140, 0.10506637, 0.31063031), (0.95922872, 0.53307513, 0.37488950))]

    def ref_magma(X):
        t = x(X, 0)*F(0.25)
        low = [M.ref_mix(p, q, t*F(4.0)) for p, q in zip(magma[0], magma[1])]
        middle = [M.ref_mix(p, q, (t - F(0.25))*F(4.0)) for p, q in zip(magma[1], magma[2])]
        high = [M.ref_mix(p, q, (t - F(0.5))*F(4.0)) for p, q in zip(magma[2], magma[3])]
        return stack([np.where(t < F(0.25), l, np.where(t < F(0.5), m, h)) for l, m, h in zip(low, middle, high)])
    add("palette_magma", "r = vec4(palette_magma(A.x*0.25), 0.0);", ref_magma, 3)
    add("parts: cos, sin of radians(A.x)", "r = vec4(cos(radians(A.x)), sin(radians(A.x)), 0.0, 0.0);", None, 2, note="scalar forms bounded in math_cases: device = host here")
    four_ = "parts: cos, sin of radians(A.x)"
    add("rotate2deg", "mat2 m = rotate2deg(A.x); r = vec4(m[0], m[1]);", lambda X, p: np.stack([p[:, 0], -p[:, 1], p[:, 1], p[:, 0]], 1), 4, uses=(four_,))
    add("rotate3deg", "r = vec4(rotate3deg(B.xyz, C.xyz, A.x), 0.0);", ref_rotate3d, 3, uses=(four_,))
    # chaotic: fract(sin(x)*39758.38): a last-bit difference in sin moves the result anywhere. Held to device = host and to [0, 1) only
    add("noise11, noise21, noise22", "r = vec4(noise11(A.x), noise21(A.xy), noise22(A.zw));", None, 4, within=(0.0, 1.0), note="chaotic: device = host and the range [0, 1) only")


prelude_rows()

BY_NAME = {row.name: row for row in ROWS}
assert len(BY_NAME) == len(ROWS), [name for name in BY_NAME if sum(r.name == name for r in ROWS) > 1][:5]
FRAGMENTS = ("float", "geometric", "matrix", "integer", "uint", "swizzle", "swizzle writes", "prelude")
PROBE_UNIFORMS = [("sampler2D", "opA"), ("sampler2D", "opB"), ("sampler2D", "opC"), ("sampler2D", "opD")]
HELPERS = """uniform int group;
uniform int column;
uint word(float high, float low) { return (uint(high) << 16) | uint(low); }
vec4 split(uvec2 v) { return vec4(float(v.x >> 16), float(v.x & 65535u), float(v.y >> 16), float(v.y & 65535u)); }
"""


def rows_of(fragment: str) -> list[Row]:
    return [row for row in ROWS if row.fragment == fragment]


def group_of(row: Row) -> int:
    return 1 + rows_of(row.fragment).index(row)


def probe_glsl(fragment: str) -> str:
    lines = [HELPERS, "void main() {",
             "    ivec2 at = ivec2(gl_FragCoord.xy);",
             "    vec4 A = texelFetch(opA, at, 0); vec4 B = texelFetch(opB, at, 0); vec4 C = texelFetch(opC, at, 0); vec4 D = texelFetch(opD, at, 0);",
             "    vec4 r = vec4(0.0);"]
    if fragment == "matrix":
        lines.append(MATRIX_PREAMBLE)
    if fragment in ("integer", "uint"):
        lines.append(INTEGER_PREAMBLE)
    lines += ["    switch (group) {",
              "        case 0: r = (column == 0) ? A : ((column == 1) ? B : ((column == 2) ? C : D)); break;"]
    for index, row in enumerate(rows_of(fragment), 1):
        tail = {"vec": "", "words": " uvec2 half_ = R.xy; if (column == 1) half_ = R.zw; r = split(half_);",
                "mat2": " r = vec4(R[column], 0.0, 0.0);", "mat3": " r = vec4(R[column], 0.0);", "mat4": " r = R[column];"}[row.kind]
        head = "uvec4 R; " if row.kind == "words" else ""
        lines.append(f"        case {index}: {{ {head}{row.body}{tail} break; }}      // {row.name}")
    lines += ["        default: break;", "    }", "    fragColor = r;", "}"]
    return "\n".join(lines) + "\n"


# ---- the inputs -------------------------------------------------------------------------------------------------------------------
INT_SPECIALS = np.array([0, 1, -1, 2, -2, 7, 255, 256, 65535, 65536, 2**31 - 1, -2**31, -2**31 + 1, 2**31, 3000000000, 2**32 - 1], np.int64) & MASK32
_cache: dict = {}


def words_to_floats(W) -> np.ndarray:
    """(n, 8) words -> (n, 16) float32: the upper and the lower 16 bits of each"""
    W = np.asarray(W, np.int64) & MASK32
    X = np.empty((len(W), 16), F)
    X[:, 0::2], X[:, 1::2] = (W >> 16).astype(F), (W & 0xffff).astype(F)
    return X


def floats_to_words(X) -> np.ndarray:
    return (X[:, 0::2].astype(np.int64) << 16) | X[:, 1::2].astype(np.int64)


def _whole(rows, rng, fill) -> np.ndarray:
    missing = -len(rows) % POINTS
    return np.concatenate([rows, fill(missing)]) if missing else rows


def _float_inputs(rng) -> tuple:
    everyday = lambda n: rng.uniform(-4, 4, (n, 16)).astype(F)                                     # noqa: E731
    blocks, special = [], []
    for slot in range(16):                                                                         # every special in every slot, everyday values around it
        block = rng.uniform(-2, 2, (len(M.SPECIALS)*4, 16)).astype(F)
        block[:, slot] = np.repeat(M.SPECIALS, 4)
        blocks.append(block)
        sweep = everyday(255*2*4)                                                                  # a stratified sweep per slot
        sweep[:, slot] = M.stratified(rng, per=4)
        blocks.append(sweep)
    # length, distance, normalize: a zero vector, subnormals, components near 2^64 (the sum of squares overflows) and 2^-75 (underflows)
    for scale in (0.0, float(M.SUB_MIN), 2.0**-140, 2.0**-75, 2.0**-64, 2.0**63, 2.0**64, 2.0**100):
        block = (rng.uniform(-4, 4, (256, 16))*scale).astype(F)
        block[:, 12:] = rng.uniform(-4, 4, (256, 4)).astype(F)
        blocks.append(block)
    # the relational functions and ==: every pair of specials in the same component (-0 with +0, NaN with NaN, inf with inf …)
    grid = np.stack(np.meshgrid(M.SPECIALS, M.SPECIALS, indexing="ij"), -1).reshape(-1, 2)
    block = everyday(len(grid))
    block[:, 0], block[:, 4] = grid[:, 0], grid[:, 1]
    blocks.append(block)
    # refract: unit-ish incident and normal vectors over the first N components (N = 1: anything in [-1, 1]), eta at, next to and
    # around the eta of k = 0. Edge points by design: not everyday ones
    for n in (1, 2, 3, 4):
        block = everyday(2560)
        for letter in (0, 4):
            v = block[:, letter:letter + n].astype(np.float64)
            block[:, letter:letter + n] = (v/(4.0 if n == 1 else np.linalg.norm(v, axis=1, keepdims=True))).astype(F)
        c = dot_([block[:, k] for k in range(n)], [block[:, 4 + k] for k in range(n)]).astype(np.float64)
        with np.errstate(all="ignore"):
            critical = (1.0/np.sqrt(np.maximum(1.0 - c*c, 1e-6))).astype(F)
        eta = critical.copy()
        for step in range(1, 3):                                                                   # critical, its two neighbours either way, and free draws
            eta[step::8] = np.nextafter(eta[step::8], F(np.inf)) if step == 1 else np.nextafter(np.nextafter(eta[step::8], F(np.inf)), F(np.inf))
        eta[3::8] = np.nextafter(eta[3::8], F(-np.inf))
        eta[4::8] = np.nextafter(np.nextafter(eta[4::8], F(-np.inf)), F(-np.inf))
        eta[5::8], eta[6::8], eta[7::8] = eta[5::8]*F(1.25), eta[6::8]*F(0.8), rng.uniform(0.3, 3.0, len(eta[7::8])).astype(F)
        block[:, 12] = eta
        blocks.append(block)
    special.append(sum(len(b) for b in blocks))
    blocks.append(everyday(32768))
    X = np.concatenate(blocks)
    X = _whole(X, rng, everyday)
    flag = np.ones(len(X), bool)
    flag[:special[0]] = False
    return X, flag


def _matrix_inputs(rng, n: int) -> tuple:
    """identity, diagonal, permutation and singular matrices, seeded matrices of float64 condition number <= 100 (the everyday points), and
    those with one special value in one slot"""
    slots = MATRIX_SLOTS[n][0]
    everyday = lambda count: rng.uniform(-4, 4, (count, 16)).astype(F)                             # noqa: E731

    def conditioned(count):
        out = []
        while sum(len(b) for b in out) < count:
            X = everyday(4*count)
            m = X[:, slots].astype(np.float64).reshape(-1, n, n)
            out.append(X[np.linalg.cond(m) <= 100])
        return np.concatenate(out)[:count]

    def with_matrix(matrices):
        X = everyday(len(matrices))
        X[:, slots] = np.asarray(matrices, F).reshape(len(matrices), n*n)
        return X

    fixed = [np.eye(n)]*8
    fixed += [np.diag(rng.uniform(-4, 4, n)) for _ in range(120)]
    fixed += [np.eye(n)[list(p)] for p in itertools.permutations(range(n))]*4
    singular = []
    for _ in range(128):
        m = rng.uniform(-4, 4, (n, n))
        which = rng.integers(0, 3)
        if which == 0:
            m[:, 1] = m[:, 0]
        elif which == 1:
            m[0, :] = 0
        else:
            m[:, n - 1] = 2*m[:, 0]
        singular.append(m)
    blocks = [with_matrix(fixed), with_matrix(singular)]
    holed = conditioned(len(M.SPECIALS)*n*n)
    for k, slot in enumerate(slots):
        holed[k*len(M.SPECIALS):(k + 1)*len(M.SPECIALS), slot] = M.SPECIALS
    blocks.append(holed)
    special = sum(len(b) for b in blocks)
    X = np.concatenate(blocks)
    X = np.concatenate([X, conditioned(POINTS - len(X))])
    flag = np.ones(len(X), bool)
    flag[:special] = False
    return X, flag


def _integer_inputs(rng) -> dict:
    rows = []
    grid = np.stack(np.meshgrid(INT_SPECIALS, INT_SPECIALS, indexing="ij"), -1).reshape(-1, 2)
    for lane in range(4):                                                                          # the full special x special grid in every lane
        block = rng.choice(INT_SPECIALS, (len(grid), 8))
        block[:, lane], block[:, 4 + lane] = grid[:, 0], grid[:, 1]
        rows.append(block)
    rows.append(rng.choice(INT_SPECIALS, (4096, 8)))
    near = rng.choice(INT_SPECIALS, (2048, 8)) + rng.integers(-3, 4, (2048, 8))
    rows.append(near & MASK32)
    W = np.concatenate(rows)
    W = np.concatenate([W, rng.integers(0, 1 << 32, (POINTS - len(W), 8), dtype=np.int64)])
    # / and %: no zero divisor, and no -2^31 among the dividends of a point that has -1 among its divisors (both as int and as uint
    # rows read the same words; every vector-scalar form pairs a.x or b.x with every component)
    D = W.copy()
    D[:, 4:][D[:, 4:] == 0] = 3
    hazard = (D[:, :4] == 1 << 31).any(1)
    for lane in range(4, 8):
        D[hazard & (D[:, lane] == MASK32), lane] = 7
    S = W.copy()                                                                                   # shift counts 0 … 31 only
    S[:, 4:] = rng.integers(0, 32, (len(S), 4))
    S[:32, 4:] = np.arange(32)[:, None]
    return {"int": W, "div": D, "shift": S}


def assert_clean(sets: dict) -> None:
    """nothing in the inputs can divide by zero, divide -2^31 by -1 or shift out of range (GLSL leaves those undefined; x86 traps)"""
    D, S = floats_to_words(sets["div"][0]), floats_to_words(sets["shift"][0])
    assert (D[:, 4:] != 0).all(), "a zero divisor"
    assert not ((D[:, :4] == 1 << 31).any(1) & (D[:, 4:] == MASK32).any(1)).any(), "-2^31 / -1"
    assert ((S[:, 4:] >= 0) & (S[:, 4:] <= 31)).all(), "a shift count outside 0 … 31"
    for row in ROWS:
        if row.inputs in ("int", "div", "shift") and any(f" {op}" in row.name for op in ("/", "%", "<<", ">>")):
            assert row.inputs == INT_INPUTS[next(op for op in ("/", "%", "<<", ">>") if f" {op}" in row.name)], row.name


def inputs() -> dict:
    """{set name: ((n, 16) float32 operands, (n,) bool: an everyday point)}; n a multiple of 256*64 (16 for the swizzles). Deterministic."""
    if _cache:
        return _cache
    seeded = lambda k: np.random.default_rng(20261 + k)                                        # noqa: E731  (a generator per set: a
    _cache["vec"] = _float_inputs(seeded(0))                                                   # change to one leaves the others, and
    for n in (2, 3, 4):                                                                        # the figures measured on them, alone)
        _cache[f"mat{n}"] = _matrix_inputs(seeded(n), n)
    for name, W in _integer_inputs(seeded(5)).items():
        _cache[name] = (words_to_floats(W), np.ones(len(W), bool))
    swizzle = np.zeros((16, 16), F)
    swizzle[:, 0:4] = np.array([1, 2, 3, 4], F) + 16*np.arange(16, dtype=F)[:, None]               # A: 1, 2, 3, 4 (+ 16 per point)
    swizzle[:, 4:8] = np.array([5, 6, 7, 8], F) + 16*np.arange(16, dtype=F)[:, None]               # B: what is written
    _cache["swizzle"] = (swizzle, np.ones(16, bool))
    assert_clean(_cache)
    return _cache


_textures: dict = {}


def reset() -> None:
    """forget the generated inputs (and the arrays cut from them)"""
    _cache.clear()
    _textures.clear()


def textures(name: str) -> list:
    """the operand set as [[A, B, C, D] per array], each (height, width, 4); the same arrays on every call, so that a renderer can
    key its uploads by them"""
    if name not in _textures:
        _textures[name] = _cut(name)
    return _textures[name]


def _cut(name: str) -> list:
    X = inputs()[name][0]
    width, height = SWIZZLE_SIZE if name == "swizzle" else (WIDTH, HEIGHT)
    arrays = X.reshape(-1, height, width, 4, 4)
    return [[np.ascontiguousarray(array[:, :, k, :]) for k in range(4)] for array in arrays]


def operands(row: Row):
    X = inputs()[row.inputs][0]
    return floats_to_words(X) if row.inputs in ("int", "div", "shift") else X


# ---- evaluation and checks ------------------------------------------------------------------------------------------------------
def evaluate(fragment: str, render: Callable) -> tuple[dict, dict]:
    """`render(group, column, [A, B, C, D], (width, height))` shades one array of operands with the fragment's probe and returns the
    (height, width, 4) float32 target. Returns ({row name: (n, columns, 4)}, {set name: (n, 16) echo})."""
    results, echo = {}, {}
    for row in rows_of(fragment):
        arrays = textures(row.inputs)
        if row.inputs not in echo:
            echo[row.inputs] = np.concatenate([np.concatenate([render(0, k, four, row.size).reshape(-1, 4) for k in range(4)], 1) for four in arrays])
        results[row.name] = np.concatenate([np.stack([render(group_of(row), k, four, row.size).reshape(-1, 4) for k in range(row.columns)], 1) for four in arrays])
    return results, echo


def check_echo(echo: dict) -> None:
    for name, got in echo.items():
        sent = inputs()[name][0]
        wrong = M.bits(got) != M.bits(sent)
        assert not wrong.any(), f"{name}: {int(wrong.sum())} of {wrong.size} echoed floats differ; first at {np.argwhere(wrong)[0].tolist()}"


def values(row: Row, got: np.ndarray) -> np.ndarray:
    """(n, columns, 4) target -> the row's (n, width) scalars (float32; words for kind words)"""
    if row.kind == "words":
        words = got[:, :, 0::2].astype(np.int64)*65536 + got[:, :, 1::2].astype(np.int64)
        return words.reshape(len(got), -1)[:, :row.width]
    if row.kind == "vec":
        return got[:, 0, :row.width]
    n = row.columns
    return got[:, :, :n].reshape(len(got), n*n)


def expected(row: Row, results: dict) -> np.ndarray:
    """the (n, columns, 4) float32 target the row must produce"""
    n = len(operands(row))
    want = np.zeros((n, row.columns, 4), F)
    if row.like:
        want[:, 0, :row.width] = results[row.like][:, 0, :row.width]
        return want
    value = np.asarray(row.ref(operands(row), *[values(BY_NAME[name], results[name]) for name in row.uses]))
    value = value.reshape(n, -1)
    if row.kind == "words":
        value = np.concatenate([value.astype(np.int64) & MASK32, np.zeros((n, 4 - value.shape[1]), np.int64)], 1)
        want[:, :, 0::2] = (value >> 16).astype(F).reshape(n, 2, 2)
        want[:, :, 1::2] = (value & 0xffff).astype(F).reshape(n, 2, 2)
    elif row.kind == "vec":
        want[:, 0, :row.width] = value.astype(F)
    else:
        size = row.columns
        want[:, :, :size] = value.astype(F).reshape(n, size, size)
    return want


def describe(row: Row, wrong: np.ndarray, got: np.ndarray, want: np.ndarray, limit=6) -> str:
    """count, row, operands and both values in hex for the first points of `wrong` ((n, columns, 4) masks and targets). The same
    message as math_cases.describe, which cannot be reused as it is: its cases have one result per point and up to three operands"""
    X = inputs()[row.inputs][0]
    points = np.flatnonzero(wrong.reshape(len(wrong), -1).any(1))
    lines = [f"{row.name}: {len(points)} of {len(wrong)} points differ   [{row.body}]"]
    for k in points[:limit]:
        column, channel = np.argwhere(wrong[k])[0]
        if row.inputs in ("int", "div", "shift"):
            sent = " ".join(f"{int(w):08x}" for w in floats_to_words(X[k:k + 1])[0])
        else:
            sent = " ".join(f"{float(v)!r}" for v in X[k])
        lines.append(f"  point {k} ({sent}), column {column} channel {channel}: got {float(got[k, column, channel])!r} [{int(M.bits(got[k, column, channel:channel + 1])[0]):08x}], "
                     f"want {float(want[k, column, channel])!r} [{int(M.bits(want[k, column, channel:channel + 1])[0]):08x}]")
    return "\n".join(lines)


def check_same(results: dict, others: dict, what: str) -> None:
    failures = []
    for name, got in results.items():
        wrong = ~M.same_bits(got, others[name])
        if wrong.any():
            failures.append(describe(BY_NAME[name], wrong, got, others[name]))
    assert not failures, f"{what}:\n" + "\n".join(failures)


def check_exact(fragment: str, results: dict) -> None:
    failures = []
    for row in rows_of(fragment):
        if row.within is not None:
            everyday, got = inputs()[row.inputs][1], values(row, results[row.name])
            inside = (got[everyday] >= row.within[0]) & (got[everyday] < row.within[1])
            if not inside.all():
                failures.append(f"{row.name}: {int((~inside).sum())} results outside [{row.within[0]}, {row.within[1]})")
        if row.ref is None and row.like is None:
            continue
        want = expected(row, results)
        wrong = ~M.same_bits(results[row.name], want)
        if wrong.any():
            failures.append(describe(row, wrong, results[row.name], want))
    assert not failures, "\n".join(failures)


def check_witness(fragment: str, results: dict, report=print) -> None:
    """the float64 witnesses: inside the mask the error keeps its derived bound, and the mask covers >= 90 % of the everyday points"""
    failures = []
    for row in rows_of(fragment):
        if row.witness is None:
            continue
        X, everyday = inputs()[row.inputs]
        error, bound, mask = row.witness(X, values(row, results[row.name]))
        coverage = float((mask & everyday).sum()/everyday.sum())
        with np.errstate(all="ignore"):
            ratio = np.where(bound[mask] > 0, error[mask]/bound[mask], np.where(error[mask] == 0, 0.0, np.inf))
        report(f"{row.name:24s} {int(mask.sum()):6d} points in the mask ({100*coverage:.1f} % of the everyday ones), largest error/bound {ratio.max():.3f}")
        if not coverage >= 0.9:
            failures.append(f"{row.name}: the mask keeps {100*coverage:.1f} % of the everyday points")
        if not (ratio <= 1).all():
            worst = np.flatnonzero(mask)[np.argmax(ratio.max(1))]
            failures.append(f"{row.name}: error {error[worst].max():.3g} > bound {bound[worst].max():.3g} at point {worst}: {X[worst].tolist()}")
    assert not failures, "\n".join(failures)


def check_inverse(results: dict, report=print) -> None:
    """max |inverse(m)*m - I| (product in float64) over the matrices of condition number <= 100"""
    for n in (2, 3, 4):
        row = BY_NAME[f"mat{n}: inverse"]
        X, conditioned = inputs()[row.inputs]
        residual = inverse_residual(X, values(row, results[row.name]), n)[conditioned]
        bound, measured = INVERSE_RESIDUAL[n]
        report(f"mat{n}: inverse residual {residual.max():.3e} (bound {bound:.3e}, the restatement's {measured})")
        assert conditioned.sum() > 8000 and residual.max() <= bound, (n, float(residual.max()), bound)


# the forms this table added to the header: a fragment that uses one, for a compile check that names it
ADDED_FORMS = {
    # (results are assigned to integer vectors: through the implicit ivec -> vec conversion the float forms would answer otherwise)
    "min/max/clamp(ivecN, ivecN)": "ivec3 a = ivec3(gl_FragCoord.xyz); ivec3 b = min(a, ivec3(2)); ivec3 c = max(a, ivec3(2)); ivec3 d = clamp(a, ivec3(1), ivec3(2)); fragColor = vec4(vec3(b + c + d), 0.0);",
    "min/max/clamp(ivecN, int)": "ivec2 a = ivec2(gl_FragCoord.xy); ivec2 b = min(a, 2); ivec2 c = max(a, 2); ivec2 d = clamp(a, 1, 2); fragColor = vec4(vec2(b + c), vec2(d));",
    "min/max/clamp(uvecN, uvecN)": "uvec4 a = uvec4(gl_FragCoord); uvec4 b = min(a, uvec4(2u)); uvec4 c = max(a, uvec4(2u)); uvec4 d = clamp(a, uvec4(1u), uvec4(2u)); fragColor = vec4(b + c + d);",
    "min/max/clamp(uvecN, uint)": "uvec2 a = uvec2(gl_FragCoord.xy); uvec2 b = min(a, 2u); uvec2 c = max(a, 2u); uvec2 d = clamp(a, 1u, 2u); fragColor = vec4(vec2(b + c), vec2(d));",
    "abs/sign(ivecN)": "ivec4 a = ivec4(gl_FragCoord); ivec4 b = abs(a); ivec4 c = sign(a); fragColor = vec4(b + c);",
    "isnan/isinf(vecN)": "bvec3 a = isnan(gl_FragCoord.xyz); bvec2 b = isinf(gl_FragCoord.xy); fragColor = vec4(vec3(a), 0.0) + vec4(vec2(b), 0.0, 0.0);",
    "outerProduct(vec4, vec4)": "mat4 m = outerProduct(gl_FragCoord, gl_FragCoord); fragColor = m[1];",
    "ivecN(bvecN), uvecN(bvecN)": "bvec2 b = lessThan(gl_FragCoord.xy, vec2(3.0)); fragColor = vec4(ivec2(b), uvec2(b));",
    "bvecN(vecN), bvecN(ivecN)": "bvec2 b = bvec2(gl_FragCoord.xy); bvec2 c = bvec2(ivec2(1, 0)); fragColor = vec4(vec2(b), vec2(c));",
    "equal/notEqual(bvecN)": "bvec2 b = lessThan(gl_FragCoord.xy, vec2(3.0)); fragColor = vec4(vec2(equal(b, b)), vec2(notEqual(b, b)));",
    "matrix += -= /=": "mat3 m = mat3(2.0); m += m; m -= mat3(1.0); m /= 2.0; m /= mat3(gl_FragCoord.x); fragColor = vec4(m[0], 1.0);",
    "matrix + - scalar, scalar + - / matrix": "mat2 m = mat2(2.0); m = (m + 1.0) - 2.0; m = 1.0 + m; m = 1.0 - m; m = 1.0/m; m += 1.0; m -= 1.0; fragColor = vec4(m[0], m[1]);",
    "matrix == !=": "mat4 m = mat4(gl_FragCoord.x); fragColor = vec4((m == m) ? 1.0 : 0.0, (m != m) ? 1.0 : 0.0, 0.0, 1.0);",
}
