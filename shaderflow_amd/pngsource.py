"""
PNG sources of a ShaderVideo, read without ffmpeg: the `MPNG` `.avi` files `pixel_format="png"` writes (mjpeg.py has the container;
its OpenDML form, `opendml=`, included: clips.py walks the `AVIX` segments of a file past 4 GiB) read back, the same from other
writers, and PNG files handed over as `bytes`. The frames stay compressed on the host and over the
link; the device inflates and unfilters them where the texture lives (csrc/png_decode_kernels.hpp defines the decode,
`sfx_png_frame` of include/shaderflow_hip.h the layout of a staged frame, mirrored here as `STAGED`).

  * `parse_header(stream)`: the signature, IHDR and every chunk up to IEND → `PngHeader` (geometry, the IDAT payloads in order), or
    ValueError naming the IHDR field and its value this decoder does not take: only 8-bit RGB (colour type 2), compression 0, filter
    method 0, no interlace are decoded — 16-bit and sub-byte depths, palette, grey, alpha and Adam7 are refused. Ancillary chunks are
    skipped, unknown critical chunks raise, and so do a stream cut short, a missing IEND, a first IDAT without a valid zlib header
    (CM = 8, a window of at most 32 KiB, FDICT = 0, the check bits) and a second picture behind IEND in one chunk.
    **Chunk CRC-32s are not checked**: a `zlib.crc32` over 5 MB a frame in the reader thread would cap a 4K clip. The Adler-32 of the
    inflated stream is checked instead, on the device (a mismatch is a status bit and the frame is not drawn).
  * `stage(stream, expected, view, name)`: the staged frame into a pinned slot: the record, one word per segment (IDAT chunk) saying
    where its bytes start in the payload, and the payload: the IDAT data concatenated, the 2-byte zlib header and the 4-byte Adler-32
    stripped (the Adler-32 goes into the record).
  * `AviReader(path)` finds the `MPNG` stream (clips.py's RIFF walk, with this FourCC).
  * `create(...)`, `paths(handle)`: the video handle of such a source (sfx_video_create_png) and its landed frames by inflate path.

The module is the codec video.py and clips.py speak to: `FORMAT`, `TITLE`, `FOURCC` and the functions above.

The device decodes a frame on one of two paths, both exact (csrc/png_decode_kernels.hpp): a wave per segment when the frame has at
least two segments and every one but the last ends in `00 00 FF FF` (`segment_path`: what this package's encoder writes — a stripe of
8 rows per IDAT — and what `Z_FULL_FLUSH` at IDAT boundaries gives), validated segment by segment, with the serial path behind it
when one does not validate; one wave for the whole stream otherwise (Pillow, ffmpeg: one serial deflate stream).
SHADERFLOW_PNG_SEGMENTS=0 / 1 forces either. Numbered-file patterns, APNG and 16-bit, grey, palette or alpha pictures are out of scope.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional

import numpy as np

from shaderflow_amd import _native as N
from shaderflow_amd.clips import AviClip

FORMAT, TITLE, FOURCC = "png", "PNG", b"MPNG"

# include/shaderflow_hip.h: sfx_png_frame, the record at the start of a staged frame (the segment table starts behind it), and SFX_PNG_*
FRAME_MAGIC = 0x4e504653                                              # "SFPN"
STAGED = np.dtype([("magic", "<u4"), ("width", "<u4"), ("height", "<u4"), ("segments", "<u4"), ("payload_bytes", "<u4"), ("payload_offset", "<u4"),
                   ("adler", "<u4"), ("reserved", "<u4")])
assert STAGED.itemsize == 32
FRAME_FIXED = STAGED.itemsize
BAD_BLOCK, BAD_STORED, BAD_LENGTHS, BAD_CODE, BAD_DISTANCE, OUT_OF_BITS, BAD_SIZE, BAD_FILTER, BAD_ADLER, BAD_DESCRIPTOR = (1 << k for k in range(10))
STATUS_BITS = {BAD_BLOCK: "a deflate block of type 3", BAD_STORED: "a stored block whose LEN and NLEN do not match", BAD_LENGTHS: "a bad code-length set",
               BAD_CODE: "a code that matches none, or a reserved length or distance symbol", BAD_DISTANCE: "a distance too far back",
               OUT_OF_BITS: "the compressed data ran out of bits", BAD_SIZE: "the stream does not inflate to the picture's size",
               BAD_FILTER: "a row's filter type above 4", BAD_ADLER: "the Adler-32 of the inflated stream is not the stream's",
               BAD_DESCRIPTOR: "a staged frame the kernels refuse"}
SIGNATURE = b"\x89PNG\r\n\x1a\n"
FLUSH = b"\x00\x00\xff\xff"                                           # an empty stored block: how a segment ends at a flush point


@dataclass
class PngHeader:
    width: int
    height: int
    payloads: list = field(default_factory=list)                      # the IDAT chunks' data, in order (views of the stream)
    end: int = 0                                                      # bytes of the stream through IEND

    @property
    def geometry(self) -> tuple:
        """What must not change inside a clip"""
        return (self.width, self.height)

    @property
    def filtered_bytes(self) -> int:
        return self.height*(1 + 3*self.width)

    @property
    def compressed(self) -> int:
        return sum(len(p) for p in self.payloads)


def parse_header(stream) -> PngHeader:
    """The chunks of one PNG stream through IEND (module docstring). Chunk CRC-32s are not checked."""
    data = memoryview(stream)
    if len(data) < 8 or bytes(data[:8]) != SIGNATURE:
        raise ValueError("not a PNG stream: no signature (89 50 4E 47 0D 0A 1A 0A) at its start")
    at, header = 8, None
    while True:
        if at + 12 > len(data):
            raise ValueError(f"PNG stream: cut short at byte {at}, before any IEND chunk" if header else "PNG stream: cut short before IHDR")
        size, kind = struct.unpack(">I4s", data[at:at + 8])
        if at + 12 + size > len(data):
            raise ValueError(f"PNG stream: the {kind!r} chunk at byte {at} is cut short ({size} bytes of data, {len(data) - at - 12} there)")
        body = data[at + 8:at + 8 + size]
        at += 12 + size
        if header is None:
            if kind != b"IHDR" or size != 13:
                raise ValueError(f"PNG stream: the first chunk is {kind!r} of {size} bytes, not IHDR of 13")
            width, height, depth, colour, compression, method, interlace = struct.unpack(">IIBBBBB", body)
            if depth != 8:
                raise ValueError(f"IHDR bit depth {depth}: only 8-bit samples are decoded")
            if colour != 2:
                names = {0: "grey", 3: "palette", 4: "grey with alpha", 6: "RGB with alpha"}
                raise ValueError(f"IHDR colour type {colour} ({names.get(colour, 'not in the standard')}): only colour type 2 (RGB) is decoded")
            if compression != 0:
                raise ValueError(f"IHDR compression method {compression}: only 0 (deflate) exists")
            if method != 0:
                raise ValueError(f"IHDR filter method {method}: only 0 (the five adaptive row filters) exists")
            if interlace != 0:
                raise ValueError(f"IHDR interlace method {interlace}{' (Adam7)' if interlace == 1 else ''}: only non-interlaced pictures are decoded")
            if width < 1 or height < 1 or height*(1 + 3*width) >= 1 << 31:
                raise ValueError(f"IHDR width {width}, height {height}: extents from 1, height x (1 + 3 width) below 2^31")
            header = PngHeader(width, height)
        elif kind == b"IDAT":
            header.payloads.append(body)
        elif kind == b"IEND":
            break
        elif kind == b"IHDR":
            raise ValueError("PNG stream: a second IHDR chunk")
        elif not kind[0] & 0x20:                                      # an upper-case first letter: critical (PLTE among them: not for colour type 2 here)
            raise ValueError(f"PNG stream: the critical chunk {kind!r} is not known to this decoder")
    header.end = at
    if header.compressed < 6:
        raise ValueError(f"PNG stream: {header.compressed} bytes of IDAT data hold no zlib stream (2 bytes of header, 4 of Adler-32)")
    first = bytes(header.payloads[0][:2]) if len(header.payloads[0]) >= 2 else b"".join(bytes(p) for p in header.payloads)[:2]
    cmf, flg = first
    if cmf & 15 != 8 or cmf >> 4 > 7 or flg & 0x20 or (cmf*256 + flg) % 31:
        raise ValueError(f"PNG stream: the first IDAT starts with {first.hex()}, no valid zlib header (CM = 8, a window of at most 32 KiB, FDICT = 0, check bits)")
    if bytes(data[at:at + 64]).lstrip(b"\0")[:8] == SIGNATURE:
        raise ValueError("PNG stream: a second picture behind the first one's IEND: two pictures in one chunk are not decoded")
    return header


def segment_path(header: PngHeader) -> bool:
    """Whether the device's production rule sends this frame down the segment path (csrc/capi_video_png.hip: png_segments_chosen): at
    least two segments, every one but the last ending in 00 00 FF FF. (The first segment loses the zlib header and the last one the
    Adler-32 when they are staged: neither touches a segment's end but the last's.)"""
    forced = os.environ.get("SHADERFLOW_PNG_SEGMENTS")
    if forced in ("0", "1"):
        return forced == "1"
    ends = _segments(header)[1][1:]
    payload = b"".join(bytes(p) for p in header.payloads)[2:-4]
    return len(ends) >= 1 and all(end >= 4 and payload[end - 4:end] == FLUSH for end in ends)


def _segments(header: PngHeader) -> tuple[int, list]:
    """(payload bytes, where each segment starts in the payload): the zlib header comes off the front, the trailer off the back"""
    total = header.compressed - 6
    starts, at = [], -2
    for payload in header.payloads:
        starts.append(min(max(at, 0), total))
        at += len(payload)
    return total, starts


def staged_bytes(header: PngHeader) -> int:
    return FRAME_FIXED + ((4*len(header.payloads) + 15) & ~15) + ((header.compressed - 6 + 15) & ~15)


def capacity_for(header: PngHeader, largest: Optional[int]) -> int:
    """The slots' capacity: what the largest frame of a clip needs when the container tells (`largest`: a whole PNG file's bytes, 12 per
    IDAT chunk among them, so a word per segment fits), else what a frame of stored blocks would (a larger one is refused when it comes)"""
    stream = largest if largest is not None else header.filtered_bytes + header.filtered_bytes//8 + 4096
    return FRAME_FIXED + 16 + ((stream + 15) & ~15)


def stage(stream, expected: Optional[PngHeader], view: np.ndarray, name: str = "frame") -> int:
    """One PNG stream → the staged frame in `view` (a 1-D uint8 array: a pinned slot); returns its bytes. `expected`: the clip's first
    header, whose geometry every frame must have."""
    header = parse_header(stream)
    if expected is not None and header.geometry != expected.geometry:
        raise ValueError(f"{name}: {header.width} x {header.height}: the clip's first frame has {expected.width} x {expected.height}")
    payload_bytes, starts = _segments(header)
    table_bytes = (4*len(starts) + 15) & ~15
    total = FRAME_FIXED + table_bytes + payload_bytes
    if total + 4 > view.size:
        raise ValueError(f"{name}: {len(stream)} bytes need a slot of {total + 4}, the slots hold {view.size}")
    # the IDAT data lands two bytes in front of the payload's place: the zlib header falls into the table's room (written below), the
    # payload where it belongs, and the trailer behind it, where it is read and wiped
    at = FRAME_FIXED + table_bytes - 2
    for payload in header.payloads:
        view[at:at + len(payload)] = np.frombuffer(payload, np.uint8)
        at += len(payload)
    tail = bytes(view[total:total + 4])
    view[total:total + 4] = 0
    view[:FRAME_FIXED + table_bytes] = 0
    fixed = view[:FRAME_FIXED].view(STAGED)[0]
    fixed["magic"], fixed["width"], fixed["height"], fixed["segments"] = FRAME_MAGIC, header.width, header.height, len(starts)
    fixed["payload_bytes"], fixed["payload_offset"], fixed["adler"] = payload_bytes, FRAME_FIXED + table_bytes, struct.unpack(">I", tail)[0]
    view[FRAME_FIXED:FRAME_FIXED + 4*len(starts)].view("<u4")[:] = starts
    return total


def describe_status(status: int) -> str:
    return "; ".join(text for bit, text in STATUS_BITS.items() if status & bit) or f"status {status}"


class AviReader(AviClip):
    """RIFF AVI (1.0, or OpenDML with its `AVIX` segments) with an `MPNG` video stream (handler or compression, in either case): one PNG file per chunk"""

    def __init__(self, path: Path):
        super().__init__(path, (sys.modules[__name__],))


def create(context_handle, boxes, temporal: int, header: PngHeader, capacity: int, slots: int) -> N.Handle:
    """The video handle of a source whose frames have `header`'s geometry: `boxes`, the texture matrix' handles as a ctypes array"""
    handle = N.Handle()
    N.check(N.lib().sfx_video_create_png(context_handle, boxes, temporal, header.width, header.height, capacity, slots, C.byref(handle)))
    return handle


def paths(handle) -> tuple[int, int]:
    """Landed frames by inflate path: (a wave per segment, one wave for the stream — chosen so or fallen back to)"""
    parallel, serial = C.c_uint64(0), C.c_uint64(0)
    N.check(N.lib().sfx_video_png_paths(handle, C.byref(parallel), C.byref(serial)))
    return parallel.value, serial.value


def device_decode(stream, context=None, segments=None) -> dict:
    """One PNG stream through the decode kernels, outside any video (the test entry sfx_png_decode): {"status", "filtered" (height,
    1 + 3 width) uint8: the inflated stream, "rgb" (height, width, 3) top row first (zeros when the status is bad), "header", "info":
    {"segments", "parallel", "fell_back"}}. `segments=False`: the serial path; `True`: the segment path (the serial path behind it
    when a segment does not validate); "auto" or None: what a video handle would choose (SHADERFLOW_PNG_SEGMENTS is honoured)."""
    if segments not in (None, False, True, "auto"):
        raise ValueError(f"segments={segments!r}: None, False, True or \"auto\"")
    context = context or N.default_context()
    header = parse_header(stream)
    view = np.zeros(capacity_for(header, len(stream)), np.uint8)
    total = stage(stream, header, view)
    filtered = np.zeros((header.height, 1 + 3*header.width), np.uint8)
    rgb = np.zeros((header.height, header.width, 3), np.uint8)
    status, words = C.c_uint32(0), (C.c_uint32*3)()
    mode = -1 if segments in (None, "auto") else int(bool(segments))
    N.check(N.lib().sfx_png_decode(context.handle, view.ctypes.data, total, header.width, header.height, mode, filtered.ctypes.data, rgb.ctypes.data,
                                   C.byref(status), words))
    return {"status": status.value, "filtered": filtered, "rgb": rgb, "header": header,
            "info": {"segments": int(words[0]), "parallel": int(words[1]), "fell_back": int(words[2])}}
