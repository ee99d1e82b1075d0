"""
The device's Motion-JPEG decode restated in numpy / float64 (csrc/jpeg_decode_kernels.hpp holds the definition): the entropy decoder is
tests/jpeg_ref.py's (`decode`: any baseline interleaved scan, the file's own tables); here are the rest — the Annex K tables for a
stream without DHT, dequantisation, the inverse DCT, rounding, the triangle filter for subsampled chroma, the fixed-point colour.

Planes travel padded to whole MCUs, as the device keeps them: Y (mcu rows*v*8, mcus per row*h*8), Cb and Cr (mcu rows*8, mcus per row*8).
"""
from __future__ import annotations

import struct

import numpy as np

import jpeg_ref as J


def with_tables(stream: bytes) -> bytes:
    """The stream with the standard's Annex K Huffman tables in front of its SOS when it has no DHT segment of its own"""
    pos, sos = 2, None
    while sos is None:
        marker, length = stream[pos + 1], struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        if marker == 0xc4:
            return stream
        if marker == 0xda:
            sos = pos
        pos += 2 + length
    tables = b""
    for selector, (bits, values) in ((0x00, J.DC_LUMINANCE), (0x10, J.AC_LUMINANCE), (0x01, J.DC_CHROMINANCE), (0x11, J.AC_CHROMINANCE)):
        tables += b"\xff\xc4" + struct.pack(">HB", 19 + len(values), selector) + bytes(bits) + bytes(values)
    return stream[:sos] + tables + stream[sos:]


def quantisers(stream: bytes) -> list[int]:
    """The quantisation table every component names in SOF0"""
    pos = 2
    while True:
        marker, length = stream[pos + 1], struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        if marker == 0xc0:
            count = stream[pos + 9]
            return [stream[pos + 12 + 3*k] for k in range(count)]
        pos += 2 + length


def decode(stream: bytes) -> dict:
    """jpeg_ref.decode's dictionary, and: "samples" — per component the values in front of the rounding, float64, padded to whole MCUs
    — and "planes", the same rounded half up and clipped, uint8"""
    info = J.decode(with_tables(stream))
    tables = quantisers(stream)
    sampling = info["sampling"] if len(tables) == 3 else [(1, 1)]
    coefficients = info["coefficients"]
    rows, columns = coefficients.shape[:2]
    samples, first = [], 0
    for component, (h, v) in enumerate(sampling):
        quant = info["quant"][tables[component]]                      # natural order
        plane = np.zeros((rows*v*8, columns*h*8))
        for b in range(h*v):
            terms = np.zeros((rows, columns, 64))
            terms[..., J.ZIGZAG] = coefficients[:, :, first + b]      # zigzag → natural
            terms = (terms*quant).reshape(rows, columns, 8, 8)
            block = np.einsum("vy,ijvu,ux->ijyx", J.DCT, terms, J.DCT) + 128.0
            by, bx = b//h, b % h
            for y in range(8):
                plane[(by*8 + y)::v*8, :].reshape(rows, columns, h*8)[:, :, bx*8:bx*8 + 8] = block[:, :, y]
        samples.append(plane)
        first += h*v
    info["samples"] = samples
    info["planes"] = [np.clip(np.floor(plane + 0.5), 0, 255).astype(np.uint8) for plane in samples]
    info["luma_sampling"] = tuple(sampling[0])
    return info


def tie_distance(samples: list[np.ndarray]) -> np.ndarray:
    """How far every value in front of the rounding is from a tie (…, 0.5, 1.5, …), all components in one vector; values the clip
    decides anyway (below -0.5 or above 255.5 by more than the band matters) count with their distance all the same"""
    values = np.concatenate([plane.reshape(-1) for plane in samples])
    return np.abs(values - np.floor(values) - 0.5)


def upsample(plane: np.ndarray, width: int, height: int, h: int, v: int) -> np.ndarray:
    """A chroma plane (padded) → (height, width) integers: the centred triangle filter, edges replicated at the component's own extent"""
    cw, ch = -(-width//h), -(-height//v)
    c = plane[:ch, :cw].astype(np.int64)
    if (h, v) == (1, 1):
        return c
    x = np.arange(width)
    j, left, right = x//2, np.clip(x//2 - 1, 0, cw - 1), np.clip(x//2 + 1, 0, cw - 1)
    odd = (x & 1).astype(bool)
    if v == 1:
        return np.where(odd, (3*c[:, j] + c[:, right] + 2) >> 2, (3*c[:, j] + c[:, left] + 1) >> 2)
    y = np.arange(height)
    near, far = y//2, np.clip(y//2 + np.where(y & 1, 1, -1), 0, ch - 1)
    s = 3*c[near] + c[far]
    return np.where(odd, (3*s[:, j] + s[:, right] + 7) >> 4, (3*s[:, j] + s[:, left] + 8) >> 4)


def to_rgb(planes: list[np.ndarray], width: int, height: int, sampling: tuple[int, int]) -> np.ndarray:
    """uint8 planes (padded) → (height, width, 3) uint8, top row first: upsampling and the 16-bit fixed-point full-range colour"""
    y = planes[0][:height, :width].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[..., None], 3, -1).astype(np.uint8)
    cb = upsample(planes[1], width, height, *sampling) - 128
    cr = upsample(planes[2], width, height, *sampling) - 128
    r = y + ((91881*cr + 32768) >> 16)
    g = y + ((-22554*cb - 46802*cr + 32768) >> 16)
    b = y + ((116130*cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def pictures(stream: bytes) -> tuple[dict, np.ndarray]:
    info = decode(stream)
    return info, to_rgb(info["planes"], info["width"], info["height"], info["luma_sampling"])


def split_planes(flat: np.ndarray, width: int, height: int, components: int, sampling: tuple[int, int]) -> list[np.ndarray]:
    """sfx_jpeg_decode's `planes` bytes → the padded planes"""
    h, v = sampling if components == 3 else (1, 1)
    columns, rows = -(-width//(8*h)), -(-height//(8*v))
    luma = flat[:rows*v*8*columns*h*8].reshape(rows*v*8, columns*h*8)
    if components == 1:
        return [luma]
    n = rows*8*columns*8
    return [luma, flat[luma.size:luma.size + n].reshape(rows*8, columns*8), flat[luma.size + n:luma.size + 2*n].reshape(rows*8, columns*8)]
