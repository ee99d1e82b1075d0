"""
The planar conversion restated in numpy (csrc/video_kernels.hpp's header comment is the definition; this file follows it line by line and
shares no code with the product): `coefficients`, `to_rgb` in int64 exactly as the rule is written, and `to_rgb_exact` in float64 with
the real-valued matrix and the same filter weights, without rounding or clipping — the witness the integer rule is held against.

A layout is anything with `subsampling` ("420", "422", "444", "mono"), `depth`, `matrix`, `range`, `chroma` and `siting`.
"""
from __future__ import annotations

from math import floor

import numpy as np

K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
SHIFT = {8: 8, 10: 14, 12: 16}


def real_coefficients(layout) -> dict:
    """ys, the four chroma gains, the luma offset and the chroma midpoint as real numbers"""
    kr, kb = K[layout.matrix]
    kg = 1.0 - kr - kb
    b = layout.depth
    if layout.range == "limited":
        ys, cs, offset = 255.0/(219.0*2**(b - 8)), 255.0/(224.0*2**(b - 8)), 16*2**(b - 8)
    else:
        ys, cs, offset = 255.0/(2**b - 1), 255.0/(2**b - 1), 0
    return dict(cy=ys, crv=2.0*(1.0 - kr)*cs, cgu=2.0*(1.0 - kb)*kb/kg*cs, cgv=2.0*(1.0 - kr)*kr/kg*cs, cbu=2.0*(1.0 - kb)*cs,
                offset=offset, mid=2**(b - 1), S=SHIFT[b])


def coefficients(layout) -> dict:
    """The five integers floor(x 2^S + 1/2), the offset, the midpoint and S"""
    real = real_coefficients(layout)
    out = dict(real)
    for name in ("cy", "crv", "cgu", "cgv", "cbu"):
        out[name] = int(floor(real[name]*2.0**real["S"] + 0.5))
    return out


def chroma_extents(layout, w: int, h: int) -> tuple[int, int]:
    if layout.subsampling == "mono":
        return 0, 0
    return (w if layout.subsampling == "444" else w//2), (h//2 if layout.subsampling == "420" else h)


def frame_bytes(layout, w: int, h: int) -> int:
    cw, ch = chroma_extents(layout, w, h)
    return (w*h + 2*cw*ch)*(2 if layout.depth > 8 else 1)


def planes(frame, w: int, h: int, layout):
    """Y, Cb, Cr as int64 (Cb, Cr None for grey), words above 2^b - 1 counted as 2^b - 1. `frame`: 1-D uint8 bytes, or uint16 samples"""
    frame = np.asarray(frame)
    if layout.depth > 8:
        samples = (frame if frame.dtype == np.uint16 else np.ascontiguousarray(frame, np.uint8).view("<u2")).astype(np.int64)
    else:
        samples = frame.astype(np.int64)
    samples = np.minimum(samples.reshape(-1), 2**layout.depth - 1)
    cw, ch = chroma_extents(layout, w, h)
    assert samples.size == w*h + 2*cw*ch, (samples.size, w, h)
    y = samples[:w*h].reshape(h, w)
    if layout.subsampling == "mono":
        return y, None, None
    return y, samples[w*h:w*h + cw*ch].reshape(ch, cw), samples[w*h + cw*ch:].reshape(ch, cw)


def axis_taps(extent: int, count: int, rule: str):
    """For every output position of an axis of `extent`: two (index, weight in quarters) taps into the chroma axis of `count` samples,
    indices clamped. `rule`: "own" (the axis is not subsampled), "nearest", "centre" or "left"."""
    at = np.arange(extent)
    i, odd = at//2, (at % 2) == 1
    if rule == "own":
        first, second, wa, wb = at, at, np.full(extent, 4), np.zeros(extent, np.int64)
    elif rule == "nearest":
        first, second, wa, wb = i, i, np.full(extent, 4), np.zeros(extent, np.int64)
    elif rule == "centre":                                             # x = 2i: (1, 3) on (c[i-1], c[i]); x = 2i + 1: (3, 1) on (c[i], c[i+1])
        first, second = np.where(odd, i, i - 1), np.where(odd, i + 1, i)
        wa, wb = np.where(odd, 3, 1), np.where(odd, 1, 3)
    elif rule == "left":                                               # x = 2i: 4 on c[i]; x = 2i + 1: (2, 2) on (c[i], c[i+1])
        first, second = i, np.where(odd, i + 1, i)
        wa, wb = np.where(odd, 2, 4), np.where(odd, 2, 0)
    else:
        raise ValueError(rule)
    return np.clip(first, 0, count - 1), wa.astype(np.int64), np.clip(second, 0, count - 1), wb.astype(np.int64)


def chroma_sixteenths(plane: np.ndarray, w: int, h: int, layout) -> np.ndarray:
    """C16 = sum of wy wx c over at most 2 x 2 chroma samples: (h, w) int64"""
    linear = layout.chroma == "linear"
    across = "own" if layout.subsampling == "444" else ((layout.siting if linear else "nearest"))
    down = "own" if layout.subsampling != "420" else ("centre" if linear else "nearest")
    xa, wxa, xb, wxb = axis_taps(w, plane.shape[1], across)
    ya, wya, yb, wyb = axis_taps(h, plane.shape[0], down)
    down_blended = wya[:, None]*plane[ya] + wyb[:, None]*plane[yb]     # the sum over wy wx c, the wy first: integers, so the same sum
    return wxa[None, :]*down_blended[:, xa] + wxb[None, :]*down_blended[:, xb]


def to_rgb(frame, w: int, h: int, layout) -> np.ndarray:
    """(h, w, 3) uint8, top row first: the integer rule, one rounding per value"""
    q = coefficients(layout)
    y, cb, cr = planes(frame, w, h, layout)
    S = q["S"]
    half = 1 << (S + 3)
    luma = 16*q["cy"]*(y - q["offset"])
    if cb is None:
        grey = (luma + half) >> (S + 4)
        values = np.stack([grey, grey, grey], axis=-1)
    else:
        d = chroma_sixteenths(cb, w, h, layout) - 16*q["mid"]
        e = chroma_sixteenths(cr, w, h, layout) - 16*q["mid"]
        values = np.stack([(luma + q["crv"]*e + half) >> (S + 4),
                           (luma - q["cgu"]*d - q["cgv"]*e + half) >> (S + 4),
                           (luma + q["cbu"]*d + half) >> (S + 4)], axis=-1)
    return np.clip(values, 0, 255).astype(np.uint8)


def intermediates_peak(layout) -> int:
    """The largest magnitude any sum of the integer rule can reach for this layout, from its own maxima"""
    q = coefficients(layout)
    top = 2**layout.depth - 1
    luma = 16*q["cy"]*max(top - q["offset"], q["offset"])
    chroma = 16*max(q["mid"], top - q["mid"])
    half = 1 << (q["S"] + 3)
    return luma + half + max(q["crv"], q["cgu"] + q["cgv"], q["cbu"])*chroma


def to_rgb_exact(frame, w: int, h: int, layout) -> np.ndarray:
    """(h, w, 3) float64, top row first: the real-valued matrix on the same filtered chroma, unrounded and unclipped"""
    q = real_coefficients(layout)
    y, cb, cr = planes(frame, w, h, layout)
    luma = q["cy"]*(y - q["offset"]).astype(np.float64)
    if cb is None:
        return np.stack([luma, luma, luma], axis=-1)
    d = chroma_sixteenths(cb, w, h, layout)/16.0 - q["mid"]
    e = chroma_sixteenths(cr, w, h, layout)/16.0 - q["mid"]
    return np.stack([luma + q["crv"]*e, luma - q["cgu"]*d - q["cgv"]*e, luma + q["cbu"]*d], axis=-1)


def error_bound(layout) -> np.ndarray:
    """Per channel: 1/2 (the one rounding) + the sum over the channel's terms of max|operand| 2^-(S+1) (each integer coefficient is
    within 1/2 of its real value times 2^S)"""
    q = coefficients(layout)
    top = 2**layout.depth - 1
    luma, chroma = max(top - q["offset"], q["offset"]), max(q["mid"], top - q["mid"])
    unit = 2.0**-(q["S"] + 1)
    if layout.subsampling == "mono":
        return np.full(3, 0.5 + luma*unit)
    return np.array([0.5 + (luma + chroma)*unit, 0.5 + (luma + 2*chroma)*unit, 0.5 + (luma + chroma)*unit])
