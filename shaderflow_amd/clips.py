"""
Containers of compressed video sources, read without ffmpeg: a memory-mapped file and where each frame lies in it. What the frames
are is a codec's business — a module (mjpegsource.py, pngsource.py) with `FORMAT` (a ShaderVideo's `format`), `TITLE` (for messages),
`FOURCC` (an AVI stream's handler or compression) and `parse_header(stream)`; this module knows no codec.

  * `Clip`: frames as `bytes`, in order, with `width`, `height`, `fps`, `format`, `largest` (the largest frame's bytes: the slots'
    capacity), `index`, and `sampling` / `components` where the codec's header has them.
  * `AviClip(path, codecs)`: RIFF AVI 1.0 and its OpenDML extension (further `RIFF 'AVIX'` chunks: files past 4 GiB), walked once for
    whichever of the codecs the file holds.
"""
from __future__ import annotations

import mmap
import struct
import warnings
from pathlib import Path
from typing import Iterator, Optional

import numpy as np


class Clip:
    """Frames of a compressed video file as `bytes`, in order, through a read-only memory map. `index`: (offset, size) of every frame.
    The file is closed behind the last frame, or by `close()`."""

    def __init__(self, path: Path, codec=None):
        self.path, self.codec = Path(path), codec
        self.file = open(self.path, "rb")
        self.map = mmap.mmap(self.file.fileno(), 0, access=mmap.ACCESS_READ) if self.path.stat().st_size else b""
        self.data = np.frombuffer(self.map, np.uint8)
        self.index: list[tuple[int, int]] = []
        self.fps: Optional[float] = None
        self.next = 0

    @property
    def format(self) -> str:
        return self.codec.FORMAT

    def describe(self) -> None:
        """width, height (sampling, components) from the first frame's header, as the codec reads it; `largest` from the index"""
        if not self.index:
            raise ValueError(f"{self.path}: no {self.codec.TITLE} frame")
        offset, size = self.index[0]
        self.header = self.codec.parse_header(bytes(self.map[offset:offset + size]))
        self.width, self.height = self.header.width, self.header.height
        for name in ("sampling", "components"):
            if hasattr(self.header, name):
                setattr(self, name, getattr(self.header, name))
        self.largest = max(size for _, size in self.index)

    def __len__(self) -> int:
        return len(self.index)

    def __iter__(self) -> Iterator[bytes]:
        return self

    def __next__(self) -> bytes:
        if self.map is None or self.next >= len(self.index):
            self.close()
            raise StopIteration
        offset, size = self.index[self.next]
        self.next += 1
        return bytes(self.map[offset:offset + size])

    def close(self) -> None:
        if self.map is not None:
            self.data = None                                          # (the array is a view of the map)
            if self.map:
                self.map.close()
            self.file.close()
            self.map = None


class AviClip(Clip):
    """RIFF AVI 1.0: `hdrl` (`strl`: `strh`, `strf`) and the `movi` list's `NNdc` / `NNdb` chunks of the first `vids` stream whose
    handler or compression is the FourCC of one of `codecs`, in either case — that codec is the clip's; `idx1` when it is there (and
    consistent), else a walk over `movi`. Audio and every other chunk are skipped. A chunk of this stream without bytes is a dropped
    frame: the picture in front of it again, so the frames behind it keep their times (nothing, in front of the first picture).
    OpenDML (what `opendml=` exports, ffmpeg and cameras write past a gigabyte or two): behind the first RIFF chunk every further
    top-level `RIFF … 'AVIX'` chunk is read too — its `LIST 'movi'` walked for the stream's chunks, `rec ` lists included; `ix##`, `JUNK`
    and everything else skipped; a last chunk cut short gives the frames that are whole; an `AVIX` chunk without a `movi` list is skipped
    with a warning. The `indx` / `ix##` indexes are not consulted: a walk touches only chunk headers, and offsets are Python integers,
    so a file past 4 GiB needs nothing special from the memory map. No such stream: LookupError, the file closed."""

    def add(self, offset: int, size: int) -> None:
        if size:
            self.index.append((offset, size))
        elif self.index:
            self.index.append(self.index[-1])                         # a dropped frame

    def __init__(self, path: Path, codecs):
        super().__init__(path)
        data = self.map
        if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
            raise ValueError(f"{self.path}: not a RIFF AVI file")
        self.stream, streams, movi, idx1 = None, 0, None, None
        by_fourcc = {codec.FOURCC: codec for codec in codecs}
        end = min(len(data), 8 + struct.unpack("<I", data[4:8])[0])

        def chunks(first: int, last: int):
            pos = first
            while pos + 8 <= last:
                fourcc, size = bytes(data[pos:pos + 4]), struct.unpack("<I", data[pos + 4:pos + 8])[0]
                yield fourcc, pos + 8, min(size, last - pos - 8)
                pos += 8 + size + (size & 1)

        for fourcc, at, size in chunks(12, end):
            if fourcc == b"LIST" and data[at:at + 4] == b"hdrl":
                for inner, inner_at, inner_size in chunks(at + 4, at + size):
                    if inner != b"LIST" or data[inner_at:inner_at + 4] != b"strl":
                        continue
                    kind = handler = compression = None
                    for leaf, leaf_at, leaf_size in chunks(inner_at + 4, inner_at + inner_size):
                        if leaf == b"strh" and leaf_size >= 28:
                            kind, handler = bytes(data[leaf_at:leaf_at + 4]), bytes(data[leaf_at + 4:leaf_at + 8])
                            scale, rate = struct.unpack("<II", data[leaf_at + 20:leaf_at + 28])
                        elif leaf == b"strf" and leaf_size >= 20:
                            compression = bytes(data[leaf_at + 16:leaf_at + 20])
                    named = [name for name in ((handler or b"").upper(), (compression or b"").upper()) if name in by_fourcc]
                    if self.stream is None and kind == b"vids" and named:
                        self.stream, self.codec = streams, by_fourcc[named[0]]
                        self.fps = rate/scale if scale and rate else None
                    streams += 1
            elif fourcc == b"LIST" and data[at:at + 4] == b"movi":
                movi = (at, size)
            elif fourcc == b"idx1":
                idx1 = (at, size)
        extensions, pos = [], end + (end & 1)                         # the `movi` lists of the OpenDML `RIFF 'AVIX'` chunks behind the first
        while pos + 12 <= len(data) and data[pos:pos + 4] == b"RIFF":
            stop = min(len(data), pos + 8 + struct.unpack("<I", data[pos + 4:pos + 8])[0])
            if data[pos + 8:pos + 12] == b"AVIX":
                found = [(at, size) for fourcc, at, size in chunks(pos + 12, stop) if fourcc == b"LIST" and data[at:at + 4] == b"movi"]
                if not found:
                    warnings.warn(f"{self.path}: the RIFF AVIX chunk at byte {pos} has no movi list: skipped", stacklevel=3)
                extensions += found
            pos = stop + (stop & 1)
        if self.stream is None:
            self.close()                                              # (the caller may open the file again, for other codecs)
            raise LookupError(f"{self.path}: no video stream with handler or compression {' or '.join(name.decode() for name in by_fourcc)}")
        if movi is None:
            raise ValueError(f"{self.path}: no movi list")
        if not self.fps:
            raise ValueError(f"{self.path}: strh gives no rate (dwRate / dwScale)")
        names = (b"%02ddc" % self.stream, b"%02ddb" % self.stream)
        if idx1 is not None:
            entries = np.frombuffer(data, np.dtype([("id", "S4"), ("flags", "<u4"), ("offset", "<u4"), ("size", "<u4")]), idx1[1]//16, idx1[0])
            mine = entries[np.isin(entries["id"], names)]
            if mine.size:
                # the offsets count from the movi fourcc, or (some writers) from the file's start: the first entry tells which
                base = movi[0] if bytes(data[movi[0] + int(mine["offset"][0]):movi[0] + int(mine["offset"][0]) + 4]) in names else 0
                found = [(base + int(offset) + 8, int(size)) for offset, size in zip(mine["offset"], mine["size"])]
                if all(offset + size <= len(data) and bytes(data[offset - 8:offset - 4]) in names for offset, size in found):
                    for entry in found:                               # (else the index does not point at this stream's chunks: walk instead)
                        self.add(*entry)

        def walk(first, last, whole=False):
            for fourcc, at, size in chunks(first, last):
                if fourcc == b"LIST" and data[at:at + 4] == b"rec ":
                    walk(at + 4, at + size, whole)
                elif fourcc in names and (not whole or size == struct.unpack("<I", data[at - 4:at])[0]):
                    self.add(at, size)
        if not self.index:
            walk(movi[0] + 4, movi[0] + movi[1])
        for at, size in extensions:                                   # (a chunk the file's end cuts short is no frame)
            walk(at + 4, at + size, True)
        self.describe()
