"""
The texture lookups of csrc/glsl.hpp ("THE RULES" there) restated for the tests: the NEAREST / LINEAR filter, the level rule, the
blend of two levels and the offset rule, in exact rational arithmetic (fractions.Fraction) rounded to binary32 once per operation —
the roundings the header's expressions have (-ffp-contract=off: every product, sum and fmaf rounds once). No fma is needed from numpy,
and "bit for bit" means what it says. log2 is the one function taken from elsewhere: the oracle's restatement of sfmath's, which
tests/test_host_math.py holds to the header's bits.

A texture is a list of levels, each (h, w, c) as numpy (row 0 = bottom); values travel as Python floats that are binary32 numbers.
"""
from __future__ import annotations

import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

from oracle import binding as O


def rn(x: Fraction) -> float:
    """the binary32 nearest to x, ties to even (subnormals included; the values here never overflow)"""
    if x == 0:
        return 0.0
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length()                              # floor(log2 |x|) or one above it
    if (n < (d << e)) if e >= 0 else ((n << -e) < d):
        e -= 1
    shift = 23 - max(e, -126)
    m = round(x*(1 << shift) if shift >= 0 else x/(1 << -shift))     # round(Fraction): half to even
    return math.ldexp(m, -shift)


def mul(a: float, b: float) -> float:
    return rn(Fraction(a)*Fraction(b))


def add(a: float, b: float) -> float:
    return rn(Fraction(a) + Fraction(b))


def sub(a: float, b: float) -> float:
    return rn(Fraction(a) - Fraction(b))


def fma(a: float, b: float, c: float) -> float:
    return rn(Fraction(a)*Fraction(b) + Fraction(c))


def wrap(i: int, size: int, repeat: bool) -> int:
    return i % size if repeat else min(max(i, 0), size - 1)


def texel(level: np.ndarray, i: int, j: int) -> tuple:
    """glsl.hpp texel(): missing components read (0, 0, 0, 1); unorm8 is c/255 correctly rounded"""
    c = [0.0, 0.0, 0.0, 1.0]
    for k, value in enumerate(level[j, i]):
        c[k] = rn(Fraction(int(value), 255)) if level.dtype == np.uint8 else float(value)
    return tuple(c)


def plain(level: np.ndarray, uv, linear: bool, repeat_x: bool, repeat_y: bool, offset=(0, 0)) -> tuple:
    """glsl.hpp texture_plain(): the filter on one level, texel coordinates moved by `offset` before they wrap"""
    h, w = level.shape[:2]
    u, v = mul(uv[0], float(w)), mul(uv[1], float(h))
    if not linear:
        return texel(level, wrap(math.floor(u) + offset[0], w, repeat_x), wrap(math.floor(v) + offset[1], h, repeat_y))
    ub, vb = sub(u, 0.5), sub(v, 0.5)
    fu, fv = math.floor(ub), math.floor(vb)
    a, b = sub(ub, float(fu)), sub(vb, float(fv))
    i0, i1 = wrap(fu + offset[0], w, repeat_x), wrap(fu + 1 + offset[0], w, repeat_x)
    j0, j1 = wrap(fv + offset[1], h, repeat_y), wrap(fv + 1 + offset[1], h, repeat_y)
    t00, t10, t01, t11 = texel(level, i0, j0), texel(level, i1, j0), texel(level, i0, j1), texel(level, i1, j1)
    na, nb = sub(1.0, a), sub(1.0, b)
    w00, w10, w01, w11 = mul(na, nb), mul(a, nb), mul(na, b), mul(a, b)
    return tuple(fma(w11, t11[k], fma(w01, t01[k], fma(w10, t10[k], mul(w00, t00[k])))) for k in range(4))


class Texture:
    """levels[0] is the texture, levels[1:] its chain (empty: none); `filter` is "linear" or "nearest", `mipmap` whether the
    minification filter is the mipmap one (LINEAR_MIPMAP_LINEAR / NEAREST_MIPMAP_NEAREST)"""

    def __init__(self, levels, filter: str, mipmap: bool, repeat_x: bool, repeat_y: bool):
        self.levels, self.linear, self.mipmap, self.repeat_x, self.repeat_y = list(levels), filter == "linear", mipmap, repeat_x, repeat_y
        self._plain = lru_cache(maxsize=None)(self._plain_uncached)

    @property
    def top(self) -> int:
        return len(self.levels) - 1

    def _plain_uncached(self, level: int, uv: tuple, linear: bool, offset: tuple) -> tuple:
        return plain(self.levels[level], uv, linear, self.repeat_x, self.repeat_y, offset)

    def at_level(self, level: int, uv, offset=(0, 0), linear=None) -> tuple:
        return self._plain(level, (float(uv[0]), float(uv[1])), self.linear if linear is None else linear, (int(offset[0]), int(offset[1])))

    def at_lambda(self, uv, lam: float, offset=(0, 0)) -> tuple:
        """glsl.hpp texture_at_lambda(): textureLod and what the bias and gradient forms end in"""
        lam = float(lam)
        if lam > self.top:
            lam = float(self.top)
        if not self.mipmap or self.top == 0 or not lam > 0.0:        # (a NaN selects level 0)
            return self.at_level(0, uv, offset)
        if not self.linear:
            return self.at_level(math.ceil(add(lam, 0.5)) - 1, uv, offset)
        below = math.floor(lam)
        f = sub(lam, float(below))
        a = self.at_level(below, uv, offset)
        if below + 1 > self.top or f == 0.0:
            return a
        b = self.at_level(below + 1, uv, offset)
        return tuple(fma(f, sub(b[k], a[k]), a[k]) for k in range(4))

    def lambda_base(self, dudx: float, dvdx: float, dudy: float, dvdy: float) -> float:
        """glsl.hpp mip_lambda_base(): 0.5*log2(rho^2), not clamped"""
        along_x, along_y = add(mul(dudx, dudx), mul(dvdx, dvdx)), add(mul(dudy, dudy), mul(dvdy, dvdy))
        rho2 = along_x if along_x > along_y else along_y
        return mul(0.5, float(O.math("log2", np.array([rho2], np.float32))[0]))

    def lambda_grad(self, dpdx, dpdy) -> float:
        """textureGrad's lambda: the gradients scaled by the extent of level 0"""
        h, w = self.levels[0].shape[:2]
        return self.lambda_base(mul(dpdx[0], float(w)), mul(dpdx[1], float(h)), mul(dpdy[0], float(w)), mul(dpdy[1], float(h)))

    def grad(self, uv, dpdx, dpdy, offset=(0, 0)) -> tuple:
        return self.at_lambda(uv, self.lambda_grad(dpdx, dpdy), offset)

    def fetch(self, p, lod: int) -> tuple:
        """texelFetch: zeros outside the level and outside the chain"""
        if not 0 <= lod <= self.top:
            return (0.0, 0.0, 0.0, 0.0)
        h, w = self.levels[lod].shape[:2]
        if not (0 <= p[0] < w and 0 <= p[1] < h):
            return (0.0, 0.0, 0.0, 0.0)
        return texel(self.levels[lod], int(p[0]), int(p[1]))

    def size(self, lod: int) -> tuple:
        lod = min(max(lod, 0), self.top)
        h, w = self.levels[0].shape[:2]
        return (max(1, w >> lod), max(1, h >> lod))
