"""
Motion-JPEG sources of a ShaderVideo, read without ffmpeg: the containers this package writes (mjpeg.py) read back, and the same from
other encoders — `.avi` (RIFF AVI 1.0, or OpenDML with its `AVIX` segments, with an `MJPG` video stream) and `.mjpeg` / `.mjpg` (JPEG
images back to back). The frames stay compressed on the host and over the link; the device decodes them where the texture lives (csrc/jpeg_decode_kernels.hpp defines the
decode, `sfx_jpeg_frame` of include/shaderflow_hip.h the layout of a staged frame, mirrored here as `STAGED`).

  * `parse_header(stream)`: a frame's marker segments up to its scan → `JpegHeader` (geometry, sampling, tables, where the scan
    starts), or ValueError naming the marker or field this decoder does not take: progressive, extended, lossless and arithmetic SOFs,
    12-bit samples, 16-bit quantisation tables, four components, sampling other than 4:2:0 / 4:2:2 (2x1) / 4:4:4 / grey,
    non-interleaved scans, two fields in one chunk. A stream without DHT segments (common in AVI `MJPG` chunks) gets the standard's
    Annex K tables.
  * `stage(stream, header, view)`: the staged frame into a pinned slot: the tables, the scan, and where every restart interval starts.
    The `FF D0…D7` pairs are found here with numpy, in the reader thread: the search is one vectorised pass over bytes the thread has
    in cache anyway (it copies them into the slot), and its result sizes the entropy kernel's launch — a kernel that searched would
    need a second launch, or a read-back, to learn how many lanes the first one wants.
  * `AviReader(path)`, `RawReader(path, fps)`: iterators of `bytes`, one JPEG stream per frame, with `width`, `height`, `fps`,
    `sampling` and `largest` (the largest frame's bytes: the slots' capacity). The map and the RIFF walk are clips.py's.
  * `create(...)`, `paths(handle)`: the video handle of such a source (sfx_video_create_mjpeg) and its landed frames by entropy path.

The module is the codec video.py and clips.py speak to: `FORMAT`, `TITLE`, `FOURCC` and the functions above.

Entropy decoding runs on the device alone. A frame whose restart intervals are short takes a lane per interval; a frame with long
intervals — a stream without restart markers is ONE interval per frame — is cut into subsequences of `SYNC_SUBSEQUENCE` bytes, a lane
each, which synchronise themselves (csrc/jpeg_decode_kernels.hpp, 1b; SHADERFLOW_JPEG_SYNC=0 / 1 forces either path). Decoding such
files on the host is out of scope.
"""
from __future__ import annotations

import ctypes as C
import struct
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional

import numpy as np

from shaderflow_amd import _native as N
from shaderflow_amd.clips import AviClip, Clip

FORMAT, TITLE, FOURCC = "mjpeg", "Motion-JPEG", b"MJPG"
# include/shaderflow_hip.h: sfx_jpeg_frame, the fixed part of a staged frame (the interval table starts behind it), and SFX_JPEG_*
FRAME_MAGIC = 0x444a4653                                              # "SFJD"
STAGED = np.dtype([("magic", "<u4"), ("scan_bytes", "<u4"), ("restart", "<u4"), ("intervals", "<u4"), ("scan_offset", "<u4"), ("components", "<u4"),
                   ("tq", "u1", 4), ("td", "u1", 4), ("ta", "u1", 4), ("reserved0", "u1", 28), ("quant", "u1", (4, 64)),
                   ("huffman", [("bits", "u1", 16), ("values", "u1", 256)], 4), ("reserved1", "u1", 128)])
assert STAGED.itemsize == 1536
FRAME_FIXED = STAGED.itemsize
BAD_CODE, BAD_RUN, BAD_RESTART, OUT_OF_BITS, BAD_DESCRIPTOR = 1, 2, 4, 8, 16
# csrc/capi_video_jpeg.hip: the subsequence path's production values — a subsequence's bytes, rounds per phase, and how many subsequences a
# frame's mean restart interval (scan bytes / intervals) must hold for the frame to take the path
SYNC_SUBSEQUENCE, SYNC_ROUNDS, SYNC_RULE = 64, 255, 4
STATUS_BITS = {BAD_CODE: "a code that matches no Huffman code", BAD_RUN: "a zero run past the block's 63rd term", BAD_RESTART: "a missing or wrong RSTn marker",
               OUT_OF_BITS: "the entropy-coded data ran out of bits", BAD_DESCRIPTOR: "a staged frame the kernels refuse"}

SOF_NAMES = {0xc1: "SOF1 (extended sequential)", 0xc2: "SOF2 (progressive)", 0xc3: "SOF3 (lossless)", 0xc5: "SOF5 (differential sequential)",
             0xc6: "SOF6 (differential progressive)", 0xc7: "SOF7 (differential lossless)", 0xc9: "SOF9 (arithmetic coding)",
             0xca: "SOF10 (arithmetic coding, progressive)", 0xcb: "SOF11 (arithmetic coding, lossless)", 0xcd: "SOF13 (arithmetic coding, differential)",
             0xce: "SOF14 (arithmetic coding, differential progressive)", 0xcf: "SOF15 (arithmetic coding, differential lossless)"}

# the standard's Annex K Huffman tables (BITS, HUFFVAL), for streams that carry none
_AC_LUMINANCE = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMINANCE = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
ANNEX_K = {
    (0, 0): (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12))),
    (0, 1): (bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12))),
    (1, 0): (bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]), _AC_LUMINANCE),
    (1, 1): (bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]), _AC_CHROMINANCE),
}


@dataclass
class JpegHeader:
    width: int
    height: int
    components: int                                                   # 3 (YCbCr) or 1 (grey)
    sampling: tuple[int, int]                                         # the luma's factors: (2, 2), (2, 1) or (1, 1)
    restart_interval: int                                             # MCUs; 0: the stream has no restart markers
    scan_start: int                                                   # the first entropy-coded byte
    quant: dict = field(default_factory=dict)                         # table → 64 bytes in zigzag order
    huffman: dict = field(default_factory=dict)                       # (class, table) → (BITS, HUFFVAL)
    selectors: list = field(default_factory=list)                     # per component (quantisation, DC, AC) table

    @property
    def geometry(self) -> tuple:
        """What must not change inside a clip"""
        return (self.width, self.height, self.components, self.sampling)

    @property
    def mcus(self) -> int:
        h, v = self.sampling
        return -(-self.width//(8*h))*-(-self.height//(8*v))


def parse_header(stream) -> JpegHeader:
    """The segments of one JPEG stream up to and including SOS (module docstring)"""
    data = stream
    if len(data) < 4 or data[0] != 0xff or data[1] != 0xd8:
        raise ValueError("not a JPEG stream: no SOI marker (FF D8) at its start")
    pos, quant, huffman, restart, frame = 2, {}, {}, 0, None
    while True:
        while pos < len(data) and data[pos] == 0xff and pos + 1 < len(data) and data[pos + 1] == 0xff:
            pos += 1                                                  # fill bytes
        if pos + 4 > len(data) or data[pos] != 0xff:
            raise ValueError(f"JPEG stream: a marker was expected at byte {pos}, before any SOS")
        marker = data[pos + 1]
        if marker == 0xd8 or 0xd0 <= marker <= 0xd7 or marker == 0x01:
            pos += 2
            continue
        if marker == 0xd9:
            raise ValueError("JPEG stream: EOI before any SOS")
        length = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        body = bytes(data[pos + 4:pos + 2 + length])
        if length < 2 or len(body) != length - 2:
            raise ValueError(f"JPEG stream: the segment of marker FF {marker:02X} at byte {pos} is cut short")
        pos += 2 + length
        if marker in SOF_NAMES:
            raise ValueError(f"{SOF_NAMES[marker]}: only baseline sequential Huffman streams (SOF0) are decoded")
        if marker == 0xcc:
            raise ValueError("DAC (arithmetic conditioning): only Huffman-coded streams are decoded")
        if marker == 0xc0:
            if frame is not None:
                raise ValueError("a second SOF0 in one stream")
            if len(body) < 6 or len(body) < 6 + 3*body[5]:
                raise ValueError(f"SOF0: a segment of {length} bytes is too short for its components")
            precision, height, width, count = struct.unpack(">BHHB", body[:6])
            if precision != 8:
                raise ValueError(f"SOF0 sample precision {precision}: only 8-bit samples are decoded")
            if count not in (1, 3):
                raise ValueError(f"SOF0 with {count} components: only 3 (YCbCr) or 1 (grey) are decoded")
            if width < 1 or height < 1:
                raise ValueError(f"SOF0 extents {width} x {height} (a height left to DNL is not read)")
            frame = (width, height, [(body[6 + 3*k], body[7 + 3*k] >> 4, body[7 + 3*k] & 15, body[8 + 3*k]) for k in range(count)])
        elif marker == 0xdb:
            while body:
                if body[0] >> 4:
                    raise ValueError("DQT with 16-bit entries (Pq = 1): only 8-bit quantisation tables are decoded")
                if (body[0] & 15) > 3 or len(body) < 65:
                    raise ValueError("DQT: a table number above 3, or a table cut short")
                quant[body[0] & 15] = body[1:65]
                body = body[65:]
        elif marker == 0xc4:
            while body:
                kind, table = body[0] >> 4, body[0] & 15
                total = sum(body[1:17])
                if kind > 1 or table > 1 or total > 256 or len(body) < 17 + total:
                    raise ValueError(f"DHT: class {kind}, table {table}, {total} codes (baseline: classes and tables 0 and 1)")
                huffman[(kind, table)] = (body[1:17], body[17:17 + total])
                body = body[17 + total:]
        elif marker == 0xdd:
            if len(body) < 2:
                raise ValueError(f"DRI: a segment of {length} bytes holds no restart interval")
            restart = struct.unpack(">H", body[:2])[0]
        elif marker == 0xda:
            break
    if frame is None:
        raise ValueError("SOS before any SOF0")
    width, height, components = frame
    if not body or len(body) < 4 + 2*body[0]:
        raise ValueError(f"SOS: a segment of {length} bytes is too short for its components")
    count = body[0]
    if count != len(components):
        raise ValueError(f"SOS with {count} of the frame's {len(components)} components: only one interleaved scan is decoded (non-interleaved scan)")
    if tuple(body[1 + 2*count:4 + 2*count]) != (0, 63, 0):
        raise ValueError(f"SOS spectral selection / approximation {tuple(body[1 + 2*count:4 + 2*count])}: a baseline scan has (0, 63, 0)")
    scan = {body[1 + 2*k]: (body[2 + 2*k] >> 4, body[2 + 2*k] & 15) for k in range(count)}
    if [cid for cid, *_ in components] != [body[1 + 2*k] for k in range(count)]:
        raise ValueError("SOS names the components in another order than SOF0, or other components")
    factors = [(h, v) for _, h, v, _ in components]
    if count == 1:
        sampling = (1, 1)                                             # a single component's scan is not interleaved: its MCU is one block
    else:
        sampling = factors[0]
        if sampling not in ((2, 2), (2, 1), (1, 1)) or factors[1:] != [(1, 1), (1, 1)]:
            raise ValueError(f"SOF0 sampling factors {factors}: only 4:2:0 (2x2), 4:2:2 (2x1) and 4:4:4 (1x1) luma over 1x1 chroma are decoded")
    header = JpegHeader(width, height, count, sampling, restart, pos, quant, huffman or dict(ANNEX_K))
    for cid, _, _, tq in components:
        td, ta = scan[cid]
        if tq not in quant:
            raise ValueError(f"SOF0 names quantisation table {tq}, which no DQT defined")
        if td > 1 or ta > 1 or (0, td) not in header.huffman or (1, ta) not in header.huffman:
            raise ValueError(f"SOS names Huffman tables DC {td} / AC {ta}, which no DHT defined")
        header.selectors.append((tq, td, ta))
    return header


def scan_end(data: np.ndarray, start: int) -> int:
    """Where the scan that starts at `start` ends: the first FF that is followed by neither 00, FF nor D0…D7 (the marker behind the
    entropy-coded data, EOI in a well-formed stream); len(data) when there is none (a truncated frame)"""
    step = 1 << 20
    for first in range(start, len(data), step):
        part = data[first:first + step + 1]
        at = np.flatnonzero(part[:-1] == 0xff)
        follower = part[at + 1]
        hit = at[(follower != 0) & (follower != 0xff) & ((follower < 0xd0) | (follower > 0xd7))]
        if hit.size:
            return first + int(hit[0])
    return len(data)


def frame_length(data: np.ndarray, start: int = 0) -> int:
    """Bytes of the JPEG stream that starts at data[start]: through the EOI behind its scan"""
    header = parse_header(memoryview(data)[start:])                   # (a view: APPn segments of any size in front of SOS cost nothing)
    end = scan_end(data, start + header.scan_start)
    return min(len(data), end + 2) - start


def staged_bytes(header: JpegHeader, stream_bytes: int) -> int:
    """An upper bound of a staged frame's bytes for a stream of `stream_bytes` bytes with this geometry"""
    intervals = -(-header.mcus//header.restart_interval) if header.restart_interval else 1
    return FRAME_FIXED + ((4*intervals + 15) & ~15) + ((stream_bytes + 15) & ~15)


def capacity_for(header: JpegHeader, largest: Optional[int]) -> int:
    """The slots' capacity: what the largest frame of a clip needs when the container tells (`largest`), else what a frame as large as
    the raw picture would (a frame larger than that is refused when it comes). The interval table is sized for a restart interval of
    one MCU: tables and restart intervals may change from frame to frame."""
    stream = largest if largest is not None else header.width*header.height*3 + 4096
    return FRAME_FIXED + ((4*header.mcus + 15) & ~15) + ((stream + 15) & ~15)


def stage(stream, expected: Optional[JpegHeader], view: np.ndarray, name: str = "frame") -> int:
    """One JPEG stream → the staged frame in `view` (a 1-D uint8 array: a pinned slot); returns its bytes. `expected`: the clip's
    first header, whose geometry and sampling every frame must have."""
    data = np.frombuffer(stream, np.uint8)
    header = parse_header(stream)
    if expected is not None and header.geometry != expected.geometry:
        raise ValueError(f"{name}: {header.width} x {header.height}, {header.components} components, sampling {header.sampling}: the clip's first frame has "
                         f"{expected.width} x {expected.height}, {expected.components}, {expected.sampling}")
    end = scan_end(data, header.scan_start)
    behind = data[end + 2:end + 2 + 64] if end + 2 <= len(data) and end < len(data) and data[end + 1] == 0xd9 else data[:0]
    second = bytes(behind).lstrip(b"\0\xff")
    if second[:1] == b"\xd8":
        raise ValueError(f"{name}: a second SOI behind the first image's EOI: two fields in one chunk (interlaced Motion-JPEG) are not decoded")
    scan = data[header.scan_start:end]
    mcus = header.mcus
    restart = header.restart_interval or mcus
    intervals = -(-mcus//restart)
    table_bytes = (4*intervals + 15) & ~15
    total = FRAME_FIXED + table_bytes + scan.size
    if total > view.size:
        raise ValueError(f"{name}: {len(data)} bytes need a slot of {total}, the slots hold {view.size}")
    view[:FRAME_FIXED] = 0
    fixed = view[:FRAME_FIXED].view(STAGED)[0]
    fixed["magic"], fixed["scan_bytes"], fixed["restart"], fixed["intervals"] = FRAME_MAGIC, scan.size, restart, intervals
    fixed["scan_offset"], fixed["components"] = FRAME_FIXED + table_bytes, header.components
    for k, (tq, td, ta) in enumerate(header.selectors):
        fixed["tq"][k], fixed["td"][k], fixed["ta"][k] = tq, td, ta
    for table, values in header.quant.items():
        fixed["quant"][table] = np.frombuffer(values, np.uint8)
    for (kind, table), (bits, values) in header.huffman.items():
        entry = fixed["huffman"][2*kind + table]                      # DC 0, DC 1, AC 0, AC 1
        entry["bits"] = np.frombuffer(bits, np.uint8)
        entry["values"][:len(values)] = np.frombuffer(values, np.uint8)
    # where the intervals start: behind every FF D0…D7 pair of the scan (an FF inside entropy-coded data is followed by 00)
    offsets = view[FRAME_FIXED:FRAME_FIXED + table_bytes].view("<u4")
    offsets[:] = 0xffffffff
    offsets[0] = 0
    if intervals > 1 and scan.size > 1:
        at = np.flatnonzero(scan[:-1] == 0xff)
        at = at[(scan[at + 1] & 0xf8) == 0xd0][:intervals - 1]
        offsets[1:1 + at.size] = at + 2
    view[FRAME_FIXED + table_bytes:total] = scan
    return total


def describe_status(status: int) -> str:
    return "; ".join(text for bit, text in STATUS_BITS.items() if status & bit) or f"status {status}"


# ---- containers (clips.py has the map and the RIFF walk; this module is their codec) ---------------------------------------------------

class RawReader(Clip):
    """`.mjpeg` / `.mjpg`: JPEG images back to back, split by walking each one's marker segments to SOS and then to the marker that
    ends its scan. A truncated last image ends the clip. The rate is not in the file: `fps=`."""

    def __init__(self, path: Path, fps: Optional[float]):
        super().__init__(path, sys.modules[__name__])
        if not fps:
            raise ValueError(f"{self.path}: a bare Motion-JPEG stream does not say its rate: give fps=")
        self.fps = float(fps)
        pos, data = 0, self.data
        while pos + 4 <= len(data):
            if data[pos] != 0xff or data[pos + 1] != 0xd8:
                if data[pos] in (0, 0xff):                            # padding between the images
                    pos += 1
                    continue
                raise ValueError(f"{self.path}: a JPEG image (FF D8) was expected at byte {pos}")
            size = frame_length(data, pos)
            if pos + size > len(data) or data[pos + size - 2] != 0xff or data[pos + size - 1] != 0xd9:
                break                                                 # cut short
            self.index.append((pos, size))
            pos += size
        self.describe()


class AviReader(AviClip):
    """RIFF AVI (1.0, or OpenDML with its `AVIX` segments) with an `MJPG` video stream (handler or compression, in either case): one JPEG stream per chunk"""

    def __init__(self, path: Path):
        super().__init__(path, (sys.modules[__name__],))


def create(context_handle, boxes, temporal: int, header: JpegHeader, capacity: int, slots: int) -> N.Handle:
    """The video handle of a source whose frames have `header`'s geometry: `boxes`, the texture matrix' handles as a ctypes array"""
    handle = N.Handle()
    N.check(N.lib().sfx_video_create_mjpeg(context_handle, boxes, temporal, header.width, header.height, header.components, header.sampling[0], header.sampling[1],
                                           capacity, slots, C.byref(handle)))
    return handle


def paths(handle) -> tuple[int, int]:
    """Landed frames by entropy path: (a lane per subsequence, a lane per restart interval)"""
    sync, serial = C.c_uint64(0), C.c_uint64(0)
    N.check(N.lib().sfx_video_jpeg_paths(handle, C.byref(sync), C.byref(serial)))
    return sync.value, serial.value


def device_decode(stream, context=None, sync=None, subsequence_bytes=None, round_budget=None) -> dict:
    """One JPEG stream through the decode kernels, outside any video (the test entries): {"status", "coefficients" (mcus, blocks per
    MCU, 64) int16 in zigzag order, "planes" the components' padded 8-bit planes as one vector, "rgb" (height, width, 3) top row
    first, "header", "sync"}. Entropy decoding: the lane-per-interval kernel (sfx_jpeg_decode; "sync" is None) unless one of the
    keywords asks for sfx_jpeg_decode_sync — `sync=True`: the subsequence path, with subsequences of `subsequence_bytes` bytes and
    `round_budget` rounds per phase (None: the production values); `sync="auto"`: whichever path a video handle would choose for this
    frame (SHADERFLOW_JPEG_SYNC is honoured); `sync=False`: the lane-per-interval kernel. "sync" is then the info record
    {"subsequences" (0: the lane-per-interval kernel ran alone), "rounds_used", "fell_back"}."""
    context = context or N.default_context()
    header = parse_header(stream)
    view = np.zeros(capacity_for(header, len(stream)), np.uint8)
    total = stage(stream, header, view)
    h, v = header.sampling
    blocks = 1 if header.components == 1 else h*v + 2
    coefficients = np.zeros((header.mcus, blocks, 64), np.int16)
    planes = np.zeros(header.mcus*64*blocks, np.uint8)
    rgb = np.zeros((header.height, header.width, 3), np.uint8)
    status = C.c_uint32(0)
    if sync is None and (subsequence_bytes is not None or round_budget is not None):
        sync = True
    if sync not in (None, False, True, "auto"):
        raise ValueError(f"sync={sync!r}: None, False, True or \"auto\"")
    info = None
    if not sync:
        N.check(N.lib().sfx_jpeg_decode(context.handle, view.ctypes.data, total, header.width, header.height, header.components, h, v,
                                        coefficients.ctypes.data, planes.ctypes.data, rgb.ctypes.data, C.byref(status)))
        if sync is False:
            info = {"subsequences": 0, "rounds_used": 0, "fell_back": 0}
    else:
        words = (C.c_uint32*3)()
        size = 0 if sync == "auto" else int(subsequence_bytes if subsequence_bytes is not None else SYNC_SUBSEQUENCE)
        N.check(N.lib().sfx_jpeg_decode_sync(context.handle, view.ctypes.data, total, header.width, header.height, header.components, h, v, size,
                                             -1 if round_budget is None else int(round_budget), coefficients.ctypes.data, planes.ctypes.data, rgb.ctypes.data,
                                             C.byref(status), words))
        info = {"subsequences": int(words[0]), "rounds_used": int(words[1]), "fell_back": int(words[2])}
    return {"status": status.value, "coefficients": coefficients, "planes": planes, "rgb": rgb, "header": header, "sync": info}
