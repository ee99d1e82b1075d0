"""
Containers of a Motion-JPEG export (`scene.main(output="clip.avi", pixel_format="mjpeg")`): the frames are encoded on the device
(csrc/jpeg_kernels.hpp) and arrive at the sink's file descriptor already framed by the read-out ring's writer thread — as bare JPEG
images back to back (`.mjpeg`, `.mjpg`, "pipe"), or as the `00dc` chunks of a RIFF AVI 1.0 file (`.avi`). `AviWriter` is the rest of
that file: the headers in front of the chunks, written with placeholders, and behind them the `idx1` index and the patched sizes.

One `vids` stream, fourcc `MJPG`. AVI 1.0 holds 4 GiB: an export that would pass it is closed, valid, at the last frame that fits and
raises (OpenDML is not written; `.mjpeg` has no such limit).
"""
from __future__ import annotations

import os
import struct
from fractions import Fraction
from typing import Iterable

SUFFIXES_AVI = (".avi",)
SUFFIXES_RAW = (".mjpeg", ".mjpg")
RIFF_LIMIT = (1 << 32) - 1


def container_of(suffix: str) -> str:
    """"avi" or "raw" by the output's suffix; anything else cannot hold an mjpeg export"""
    suffix = suffix.lower()
    if suffix in SUFFIXES_AVI:
        return "avi"
    if suffix in SUFFIXES_RAW:
        return "raw"
    raise ValueError(f"pixel_format 'mjpeg' writes '.avi' (RIFF AVI, fourcc MJPG) or '.mjpeg' / '.mjpg' (the JPEG images back to back), not {suffix!r}")


def check_quality(quality) -> int:
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_quality {quality!r}: an integer from 1 to 100")
    return quality


def chunk(payload: bytes) -> bytes:
    """A frame as the ring's writer frames it: fourcc, little-endian size, payload, a pad byte to an even length"""
    return b"00dc" + struct.pack("<I", len(payload)) + payload + b"\0"*(len(payload) & 1)


class AviWriter:
    """The file around the `00dc` chunks. `begin()` writes the headers through the descriptor; the chunks follow (from the ring's
    writer, or `add()`); `finish(sizes)` appends `idx1` and patches the frame count and the sizes."""

    def __init__(self, fileno: int, width: int, height: int, fps: float, limit: int = RIFF_LIMIT):
        self.fileno, self.width, self.height, self.limit = fileno, width, height, limit
        rate = Fraction(fps).limit_denominator(100000)
        self.rate, self.scale = rate.numerator, rate.denominator
        self.sizes: list[int] = []

    def headers(self, frames: int, movi_bytes: int, riff_bytes: int, largest: int) -> bytes:
        pixels = self.width*self.height*3
        avih = struct.pack("<14I", round(1e6*self.scale/self.rate), 0, 0, 0x10, frames, 0, 1, largest, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, frames, largest, 0xffffffff, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", pixels, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        return (b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl +
                b"LIST" + struct.pack("<I", movi_bytes) + b"movi")

    def begin(self) -> None:
        self.start = len(self.headers(0, 0, 0, 0))                     # where the first chunk goes
        os.write(self.fileno, self.headers(0, 0, 0, 0))

    def add(self, payload: bytes) -> None:
        os.write(self.fileno, chunk(payload))
        self.sizes.append(len(payload))

    def finish(self, sizes: Iterable[int] | None = None) -> None:
        sizes = list(self.sizes if sizes is None else sizes)
        # RIFF's size field counts everything behind it: the headers less 8, the chunks, idx1's 8 + 16 per frame
        fit, chunks = 0, 0
        for size in sizes:
            more = 8 + size + (size & 1)
            if self.start - 8 + chunks + more + 8 + 16*(fit + 1) > self.limit:
                break
            fit, chunks = fit + 1, chunks + more
        os.ftruncate(self.fileno, self.start + chunks)
        os.lseek(self.fileno, 0, os.SEEK_END)
        index, offset = bytearray(), 4                                  # offsets count from the `movi` fourcc
        for size in sizes[:fit]:
            index += struct.pack("<4sIII", b"00dc", 0x10, offset, size)
            offset += 8 + size + (size & 1)
        os.write(self.fileno, b"idx1" + struct.pack("<I", len(index)) + bytes(index))
        riff = self.start - 8 + chunks + 8 + len(index)
        os.pwrite(self.fileno, self.headers(fit, 4 + chunks, riff, max(sizes[:fit], default=0)), 0)
        if fit < len(sizes):
            raise RuntimeError(f"an AVI 1.0 file holds 4 GiB: closed at frame {fit} of {len(sizes)}; write '.mjpeg' (no container, no limit) for the whole export")
