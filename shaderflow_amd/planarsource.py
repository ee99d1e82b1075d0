"""
Planar video sources of any layout the device converts (no reference equivalent: the reference pipes every file through ffmpeg).

A `PlanarLayout` says how a frame's planes Y, Cb, Cr lie in memory and how they become RGB: subsampling (420, 422, 444, mono), depth
(8, 10, 12; deeper than 8: little-endian 16-bit words), matrix (bt601, bt709, bt2020), range (limited, full) and the chroma filter
(nearest or linear, sited centre or left). The conversion itself is `k_video_planar`'s (csrc/video_kernels.hpp, whose header comment is
the definition; tests/planar_ref.py restates it) — this project's own, **unpinned against swscale**.

`parse_y4m` reads a YUV4MPEG2 stream header into such fields; `PlanarReader` holds the frame loop of `.y4m` and raw planar files, which
`video.PlanarFile` (the 8-bit 4:2:0 front, kept for its callers) and `PlanarClip` (every layout; what `ShaderVideo` opens) share.

Y4M tags read: `C420` / `C420jpeg` (4:2:0, chroma sited centre), `C420mpeg2` (sited left), `C420paldv` (its co-sited, line-alternating
chroma is not interpolated: `nearest` only), `C422` (sited left), `C444`, `Cmono`, the three colour layouts with `p10` / `p12`, and
`XCOLORRANGE=FULL` / `LIMITED`. Refused, naming the tag: interlace, `C444alpha`, `C411`, 9 / 14 / 16 bit samples and deep grey.
"""
from __future__ import annotations

import re
from pathlib import Path
from typing import Optional

import numpy as np
from attrs import define

SUBSAMPLINGS = ("420", "422", "444", "mono")                          # their indices are the SFX_PLANAR_* numbers (include/shaderflow_hip.h)
MATRICES = ("bt601", "bt709", "bt2020")
RANGES = ("limited", "full")
FILTERS = ("nearest", "linear")
SITINGS = ("centre", "left")
DEPTHS = (8, 10, 12)
FORMATS = {"yuv420p": "420", "yuv422p": "422", "yuv444p": "444", "gray": "mono"}
FORMAT_NAMES = ("gray",) + tuple(name + suffix for name in ("yuv420p", "yuv422p", "yuv444p") for suffix in ("", "10le", "12le"))


@define(frozen=True)
class PlanarLayout:
    subsampling: str = "420"
    depth: int = 8
    matrix: str = "bt601"
    range: str = "limited"
    chroma: str = "nearest"
    siting: str = "centre"

    def __attrs_post_init__(self):
        for field, value, known in (("subsampling", self.subsampling, SUBSAMPLINGS), ("depth", self.depth, DEPTHS), ("yuv_matrix", self.matrix, MATRICES),
                                    ("yuv_range", self.range, RANGES), ("chroma", self.chroma, FILTERS), ("siting", self.siting, SITINGS)):
            if value not in known:
                raise ValueError(f"planar layout: {field} {value!r} is none of {', '.join(map(str, known))}")
        if self.subsampling == "mono" and self.depth != 8:
            raise ValueError(f"planar layout: grey frames are read at 8 bits, not {self.depth}")

    @classmethod
    def from_format(cls, name: str, **fields) -> "PlanarLayout":
        """The layout of a pixel-format name: yuv420p / yuv422p / yuv444p, those with 10le or 12le, or gray (`i420`: yuv420p)"""
        found = re.fullmatch(r"(yuv4[24][024]p|gray)(?:(10|12)le)?", "yuv420p" if name == "i420" else str(name))
        if not found or found.group(1) not in FORMATS or (found.group(1) == "gray" and found.group(2)):
            raise ValueError(f"planar format {name!r}: one of {', '.join(FORMAT_NAMES)}")
        fields.setdefault("siting", "left" if FORMATS[found.group(1)] == "422" else "centre")     # (as the Y4M tags C422 and C420jpeg)
        return cls(subsampling=FORMATS[found.group(1)], depth=int(found.group(2) or 8), **fields)

    @property
    def sample_bytes(self) -> int:
        return 2 if self.depth > 8 else 1

    @property
    def is_i420(self) -> bool:
        """The layout k_video_frame<SFX_VIDEO_I420> converts: such a source keeps that kernel, and `format == "i420"`"""
        return (self.subsampling, self.depth, self.matrix, self.range, self.chroma) == ("420", 8, "bt601", "limited", "nearest")

    def chroma_extents(self, width: int, height: int) -> tuple[int, int]:
        """(width, height) of either chroma plane; (0, 0) for grey"""
        if self.subsampling == "mono":
            return 0, 0
        return (width if self.subsampling == "444" else width//2), (height//2 if self.subsampling == "420" else height)

    def check_extents(self, width: int, height: int) -> None:
        if width < 1 or height < 1:
            raise ValueError(f"a planar source needs extents of at least 1, not {width} x {height}")
        if self.subsampling == "420" and (width % 2 or height % 2):
            raise ValueError(f"a 4:2:0 source needs even extents, not {width} x {height}")
        if self.subsampling == "422" and width % 2:
            raise ValueError(f"a 4:2:2 source needs an even width, not {width} x {height}")

    def frame_bytes(self, width: int, height: int) -> int:
        cw, ch = self.chroma_extents(width, height)
        return (width*height + 2*cw*ch)*self.sample_bytes

    def describe(self) -> str:
        name = "gray" if self.subsampling == "mono" else f"yuv{self.subsampling}p" + (f"{self.depth}le" if self.depth > 8 else "")
        filtered = self.chroma + (f" ({self.siting})" if self.chroma == "linear" and self.subsampling in ("420", "422") else "")
        return f"{name} {self.matrix} {self.range} {filtered}"

    def native(self):
        """sfx_planar_layout for sfx_video_create_planar"""
        from shaderflow_amd import _native as N
        return N.PlanarLayout(SUBSAMPLINGS.index(self.subsampling), self.depth, MATRICES.index(self.matrix), RANGES.index(self.range),
                              FILTERS.index(self.chroma), SITINGS.index(self.siting))


Y4M_COLOUR = {"420": ("420", "centre"), "420jpeg": ("420", "centre"), "420mpeg2": ("420", "left"), "420paldv": ("420", "centre"),
              "422": ("422", "left"), "444": ("444", "centre"), "mono": ("mono", "centre")}


def parse_y4m(line: bytes) -> tuple[int, int, float, dict]:
    """(width, height, fps, fields) of a YUV4MPEG2 stream header. `fields`: `subsampling`, `depth`, `siting`, `range` (None without an
    XCOLORRANGE tag), `nearest_only` (the tag whose chroma cannot be interpolated, or None) and `tags` (letter → the token it came as).
    ValueError names the tag this package does not read."""
    tokens = line.rstrip(b"\n").decode("ascii", "replace").split(" ")
    if tokens[0] != "YUV4MPEG2":
        raise ValueError(f"not a YUV4MPEG2 stream: it begins with {tokens[0][:16]!r}")
    width = height = fps = None
    fields = dict(subsampling="420", depth=8, siting="centre", range=None, nearest_only=None, tags={})
    for token in filter(None, tokens[1:]):
        tag, value = token[0], token[1:]
        if tag == "W":
            width = int(value)
        elif tag == "H":
            height = int(value)
        elif tag == "F":
            num, _, den = value.partition(":")
            fps = float(int(num))/float(int(den or 1))
        elif tag == "I" and value != "p":
            raise ValueError(f"y4m tag {token!r}: only progressive frames (Ip) are read")
        elif tag == "C":
            found = re.fullmatch(r"(420|422|444)p(\d+)", value)
            colour, depth = (found.group(1), int(found.group(2))) if found else (value, 8)
            if colour not in Y4M_COLOUR or depth not in DEPTHS:
                raise ValueError(f"y4m tag {token!r}: read are C420, C420jpeg, C420mpeg2, C420paldv, C422, C444 (those three also p10 and p12) and Cmono")
            fields["subsampling"], fields["siting"] = Y4M_COLOUR[colour]
            fields["depth"], fields["nearest_only"] = depth, (token if colour == "420paldv" else None)
            fields["tags"]["C"] = token
        elif tag == "X" and value.upper() in ("COLORRANGE=FULL", "COLORRANGE=LIMITED"):      # (other X tags are comments)
            fields["range"] = value.upper().partition("=")[2].lower()
            fields["tags"]["X"] = token
    if not (width and height and fps) or width < 1 or height < 1 or fps <= 0:
        raise ValueError(f"y4m header without W, H and F: {line[:80]!r}")
    if fields["subsampling"] == "420" and (width % 2 or height % 2):
        raise ValueError(f"y4m W{width} H{height}: 4:2:0 frames need even extents")
    if fields["subsampling"] == "422" and width % 2:
        raise ValueError(f"y4m W{width} H{height}: 4:2:2 frames need an even width")
    return width, height, fps, fields


class PlanarReader:
    """Frames of a `.y4m` or raw planar file, in order: an iterator of 1-D uint8 arrays of `frame_bytes` bytes, and `readinto(view)` for
    a caller with a buffer of its own (the sequence's pinned slots: no intermediate array). A truncated last frame ends the clip, as a
    short read ends iter_video_frames. A subclass says what a header means (`_header`) and how large a frame is (`_frame_bytes`)."""

    def __init__(self, path: Path, width: Optional[int] = None, height: Optional[int] = None, fps: Optional[float] = None):
        self.path, self.y4m = Path(path), Path(path).suffix.lower() == ".y4m"
        self.file = open(self.path, "rb", buffering=0)
        try:
            if self.y4m:
                width, height, fps = self._header(self._line(limit=4096))
            self.width, self.height, self.fps = width, height, fps
            self.frame_bytes = self._frame_bytes()
        except BaseException:
            self.file.close()
            raise

    def _header(self, line: bytes) -> tuple[int, int, float]:
        raise NotImplementedError

    def _frame_bytes(self) -> int:
        raise NotImplementedError

    def _line(self, limit: int = 256) -> bytes:
        """Up to and including the next newline (unbuffered file: a few bytes at a time only for these short lines)"""
        line = bytearray()
        while len(line) < limit and (byte := self.file.read(1)):
            line += byte
            if byte == b"\n":
                break
        return bytes(line)

    def readinto(self, view) -> bool:
        """The next frame into `view` (a writable buffer of frame_bytes bytes); False at the end of the clip"""
        if self.file is None:
            return False
        if self.y4m:
            line = self._line()
            if not line:
                return self._end()
            if not (line.startswith(b"FRAME") and line.endswith(b"\n")):
                raise ValueError(f"{self.path}: expected a FRAME line, found {line[:32]!r}")
            if any(token[:1] == b"I" for token in line[5:].split()):
                raise ValueError(f"{self.path}: frame tag {line[5:].strip()!r}: per-frame interlacing is not read")
        target, got = memoryview(view).cast("B"), 0
        while got < self.frame_bytes:
            count = self.file.readinto(target[got:])
            if not count:
                return self._end()                                    # a truncated last frame ends the clip
            got += count
        return True

    def _end(self) -> bool:
        self.file.close()
        self.file = None
        return False

    def __iter__(self):
        return self

    def __next__(self) -> np.ndarray:
        frame = np.empty(self.frame_bytes, np.uint8)
        if not self.readinto(frame):
            raise StopIteration
        return frame


class PlanarClip(PlanarReader):
    """A `.y4m` file (the layout is its header's) or a raw planar file of `format` (a name `PlanarLayout.from_format` takes; with
    width, height and fps given). `matrix` and `chroma` are the caller's — no Y4M tag says them; `range`: None for the file's tag,
    else limited. `layout` is what its frames are."""

    def __init__(self, path: Path, width: Optional[int] = None, height: Optional[int] = None, fps: Optional[float] = None,
                 format: Optional[str] = None, matrix: str = "bt601", range: Optional[str] = None, chroma: str = "nearest"):
        self._given = dict(matrix=matrix, range=range, chroma=chroma)
        self.layout = None if Path(path).suffix.lower() == ".y4m" else PlanarLayout.from_format(format or "yuv420p", matrix=matrix, range=range or "limited", chroma=chroma)
        PlanarReader.__init__(self, path, width, height, fps)

    def _header(self, line: bytes) -> tuple[int, int, float]:
        width, height, fps, fields = parse_y4m(line)
        given = self._given
        if given["chroma"] == "linear" and fields["nearest_only"]:
            raise ValueError(f"{self.path}: y4m tag {fields['nearest_only']!r}: its chroma is not interpolated, chroma=\"nearest\" only")
        self.layout = PlanarLayout(subsampling=fields["subsampling"], depth=fields["depth"], matrix=given["matrix"],
                                   range=given["range"] or fields["range"] or "limited", chroma=given["chroma"], siting=fields["siting"])
        return width, height, fps

    def _frame_bytes(self) -> int:
        if not all((self.width, self.height, self.fps)):
            raise ValueError(f"{self.path}: raw planar video needs width=, height= and fps=")
        self.layout.check_extents(self.width, self.height)
        return self.layout.frame_bytes(self.width, self.height)
