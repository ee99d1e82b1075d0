"""
Containers of a Motion-JPEG export (`scene.main(output="clip.avi", pixel_format="mjpeg")`): the frames are encoded on the device
(csrc/jpeg_kernels.hpp) and arrive at the sink's file descriptor already framed by the read-out ring's writer thread — as bare JPEG
images back to back (`.mjpeg`, `.mjpg`, "pipe"), or as the `00dc` chunks of a RIFF AVI 1.0 file (`.avi`). `AviWriter` is the rest of
that file: the headers in front of the chunks, written with placeholders, and behind them the `idx1` index and the patched sizes.

One `vids` stream, fourcc `MJPG` — or `MPNG` (`pixel_format="png"`: every `00dc` chunk a complete PNG file made by csrc/png_kernels.hpp; the
same file otherwise, sound track included; ffmpeg and VLC map that fourcc to their PNG decoders). AVI 1.0 holds 4 GiB: an export that
would pass it is closed, valid, at the last frame that fits and raises (`.mjpeg` has no such limit) — unless the file is written as
OpenDML (below), which holds 256 segments of 1 GiB by default and of 2 GiB at the most.

With a `SoundTrack` (`scene.main(..., sound_track=True)`) the file has a second stream, `auds`, and this is its definition:

  samples   PCM signed 16-bit little-endian, interleaved, the clip's own channel count and sample rate;
            `pcm_s16(x) = clip(rint(float64(x)*32768), -32768, 32767)`, ties to even, NaN → 0 (a 16-bit WAV source round-trips bit for bit:
            audio.reader divides by 32768)
  schedule  the writer's fps is the rational rate/scale; `a(k) = min(N, (k*samplerate*scale) // rate)` in integers, N the clip's sample
            frames; the chunk behind video frame k holds sample frames [a(k), a(k+1)); an empty range writes no chunk; a longer clip is
            cut at a(frames), a shorter one simply ends
  file      avih: two streams, AVIF_ISINTERLEAVED beside AVIF_HASINDEX; a second `strl` (strh `auds`, handler 0, scale 1, rate the sample
            rate, length the sample frames written, sample size nBlockAlign, suggested buffer the largest audio chunk; strf the 16-byte
            PCMWAVEFORMAT); `00dc` then `01wb` frame by frame; `idx1` lists the chunks of both streams in file order, and the 4 GiB
            accounting counts them all

OpenDML (AVI 2.0; `AviWriter(..., opendml=budget)`, `scene.main(..., opendml=True)`) is opt-in; without it every file is byte for byte the
one above. This is its definition, stated from the OpenDML 1.02 text; ffmpeg's and VLC's readers follow `qwOffset`, so the `ix##`
chunks may sit at the file's end. Nothing here opens an AVI in a player: the layout is pinned by tests/odml_ref.py, not against one.

  segments  `run(j)` is the bytes frame j puts into the file: its `00dc` chunk with the pad byte, plus its `01wb` chunk with the pad byte
            if it has one. `start` is where the first chunk goes, `budget` the bytes a RIFF chunk may span (SEGMENT_BYTES = 1 GiB by
            default, ffmpeg's; 4 096 … 2^31 allowed):

                pos = start; seg_start = 0; in_seg = 0
                for every frame j:
                    if in_seg > 0 and pos + run(j) - seg_start > budget:
                        a gap of 24 bytes at pos; seg_start = pos; pos += 24; in_seg = 0; j is a cut
                    pos += run(j); in_seg += 1

            (`segment_cuts`; csrc/ring_segments.hpp is the same rule in the ring's writer thread.) A frame stays with its audio and a
            segment always takes at least one frame. Segment 0 is the `RIFF 'AVI '` chunk from byte 0; every gap becomes
            `RIFF <size> AVIX LIST <size> movi`. So every RIFF chunk but the last spans at most `budget` bytes, unless one frame alone
            is larger; the last passes it by its index chunks, 8 bytes per chunk and 32 per index chunk.
  hdrl      in each `strl`, behind `strf`, an `indx` super index with room for SUPER_ENTRIES = 256 entries: the 24-byte header
            wLongsPerEntry 4, bIndexSubType 0, bIndexType 0 (index of indexes), nEntriesInUse, dwChunkId (`00dc` / `01wb`), 12
            reserved bytes; then 256 entries of qwOffset (the file offset of an `ix##` chunk's header), dwSize (that chunk's bytes,
            its 8-byte header included), dwDuration (the segment's frames; audio: its sample frames); unused entries are zero.
            Behind the streams a `LIST 'odml'` with `dmlh`: 248 bytes, the first four dwTotalFrames (all frames of the file), the
            rest zero. `avih.dwTotalFrames` counts the frames of the first RIFF chunk only; `strh.dwLength` counts all frames (audio:
            all sample frames). The headers' size is fixed once `opendml` and the track are known.
  indexes   no `idx1`: `indx` is the index and AVIF_HASINDEX stays set; a player that knows only AVI 1.0 walks the first `movi`.
            Behind the last data chunk, still inside the last segment's `movi`, one standard index chunk per segment and stream that
            has chunks there (`ix00`, `ix01`; segment by segment, video first): the 24-byte header wLongsPerEntry 2, bIndexSubType 0,
            bIndexType 1, nEntriesInUse, dwChunkId, qwBaseOffset (the file offset of that segment's `movi` fourcc), 4 reserved
            bytes; then 8-byte entries dwOffset (from the base to the chunk's DATA, not its header) and dwSize (the data bytes; bit 31
            clear: every frame is a key frame). A segment without audio chunks (the track has ended) gets no `ix01` and no
            super-index entry.
  limits    every RIFF size is below 2^32, or `finish()` raises. An export that needs more than 256 segments is closed, valid, at the
            last frame of segment 255 and raises, naming the frame: a larger segment size holds the whole export.
"""
from __future__ import annotations

import os
import struct
from fractions import Fraction
from typing import Iterable, Optional

import numpy as np

SUFFIXES_AVI = (".avi",)
SUFFIXES_RAW = (".mjpeg", ".mjpg")
RIFF_LIMIT = (1 << 32) - 1
SEGMENT_BYTES = 1 << 30                  # an OpenDML file's RIFF chunks span this at the most, by default
SEGMENT_RANGE = (4096, 1 << 31)
SUPER_ENTRIES = 256                      # room in a stream's `indx` super index: the most segments of a file
GAP_BYTES = 24                           # `RIFF size AVIX LIST size movi`


def container_of(suffix: str, pixel_format: str = "mjpeg") -> str:
    """"avi" or "raw" by the output's suffix; anything else cannot hold an mjpeg export. A png export has the one container"""
    suffix = suffix.lower()
    if suffix in SUFFIXES_AVI:
        return "avi"
    if pixel_format == "png":
        raise ValueError(f"pixel_format 'png' writes '.avi' (RIFF AVI, fourcc MPNG: every frame a PNG file) or \"pipe\" (the PNG files back to back), not {suffix!r}")
    if suffix in SUFFIXES_RAW:
        return "raw"
    raise ValueError(f"pixel_format 'mjpeg' writes '.avi' (RIFF AVI, fourcc MJPG) or '.mjpeg' / '.mjpg' (the JPEG images back to back), not {suffix!r}")


def check_quality(quality) -> int:
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg_quality {quality!r}: an integer from 1 to 100")
    return quality


def check_opendml(opendml) -> Optional[int]:
    """`opendml=`: None / False (AVI 1.0), True (SEGMENT_BYTES) or the segment size in bytes"""
    if opendml is None or opendml is False:
        return None
    if opendml is True:
        return SEGMENT_BYTES
    if not isinstance(opendml, int) or not SEGMENT_RANGE[0] <= opendml <= SEGMENT_RANGE[1]:
        raise ValueError(f"opendml {opendml!r}: True (segments of {SEGMENT_BYTES} bytes) or a segment size from {SEGMENT_RANGE[0]} to {SEGMENT_RANGE[1]} bytes")
    return opendml


def run_bytes(size: int, sound: int = 0) -> int:
    """run(j): the bytes a frame of `size` payload bytes puts into the file, with the `sound` payload bytes of its audio chunk"""
    return 8 + size + (size & 1) + ((8 + sound + (sound & 1)) if sound else 0)


class Segments:
    """The segment rule of an OpenDML file, frame by frame (csrc/ring_segments.hpp is the same, in the ring's writer thread)"""

    def __init__(self, start: int, budget: int, gap: int = GAP_BYTES):
        self.pos, self.seg_start, self.in_seg, self.budget, self.gap = start, 0, 0, budget, gap

    def cut(self, run: int) -> bool:
        """The next frame takes `run` bytes: does a gap go in front of it?"""
        gap_first = self.in_seg > 0 and self.pos + run - self.seg_start > self.budget
        if gap_first:
            self.seg_start, self.pos, self.in_seg = self.pos, self.pos + self.gap, 0
        self.pos, self.in_seg = self.pos + run, self.in_seg + 1
        return gap_first


def segment_cuts(runs: Iterable[int], start: int, budget: int) -> list[int]:
    """The frames in front of which a gap goes: `runs[j]` the bytes of frame j, the first at `start`, RIFF chunks of `budget` at the most"""
    rule = Segments(start, budget)
    return [j for j, run in enumerate(runs) if rule.cut(run)]


class Layout:
    """An OpenDML file's layout: `fit` frames are kept (all, unless SUPER_ENTRIES segments do not hold them), `cuts` the frames in front
    of which a gap lies; per segment `spans` (where its RIFF chunk begins, where it ends), `movis` (the offset of its `movi` fourcc) and
    `frames` (first, behind the last); `data_end` is where the index chunks begin and `tail` their bytes; `supers[stream]` the entries
    (qwOffset, dwSize, dwDuration) of that stream's super index; `first` the frames of segment 0, `samples` the audio's sample frames"""


def opendml_layout(sizes, audio, start: int, budget: int, block: int = 1) -> Layout:
    """The layout of `sizes` video payloads with `audio` payload bytes behind each (0: no chunk; None: no track), the first chunk at
    `start`, segments of `budget` bytes, `block` the audio's bytes per sample frame. Pure: no file is touched."""
    sizes = [int(size) for size in sizes]
    audio = [0]*len(sizes) if audio is None else [int(sound) for sound in audio]
    plan = Layout()
    runs = [run_bytes(size, sound) for size, sound in zip(sizes, audio)]
    cuts = segment_cuts(runs, start, budget)
    plan.fit = cuts[SUPER_ENTRIES - 1] if len(cuts) >= SUPER_ENTRIES else len(sizes)
    plan.cuts = cuts[:SUPER_ENTRIES - 1]
    bounds = [0, *plan.cuts, plan.fit]
    plan.frames = list(zip(bounds[:-1], bounds[1:]))
    plan.spans, plan.movis, plan.supers, tail = [], [], [[], []], bytearray()
    entries = []                                                       # per segment: per stream, the (dwOffset, dwSize) pairs
    pos = start
    for number, (first, last) in enumerate(plan.frames):
        begin = 0 if number == 0 else pos
        pos += GAP_BYTES if number else 0
        movi = pos - 4
        video, sound_entries = [], []
        for size, sound in zip(sizes[first:last], audio[first:last]):
            video.append((pos + 8 - movi, size))
            pos += 8 + size + (size & 1)
            if sound:
                sound_entries.append((pos + 8 - movi, sound))
                pos += 8 + sound + (sound & 1)
        plan.spans.append([begin, pos])
        plan.movis.append(movi)
        entries.append((video, sound_entries))
    plan.data_end = pos
    for number, streams in enumerate(entries):
        for stream, found in enumerate(streams):
            if not found:
                continue
            body = struct.pack("<HBBI4sQI", 2, 0, 1, len(found), (b"00dc", b"01wb")[stream], plan.movis[number], 0)
            body += b"".join(struct.pack("<II", offset, size) for offset, size in found)
            duration = len(found) if stream == 0 else sum(size for _, size in found)//block
            plan.supers[stream].append((plan.data_end + len(tail), 8 + len(body), duration))
            tail += (b"ix00", b"ix01")[stream] + struct.pack("<I", len(body)) + body
    plan.tail = bytes(tail)
    plan.spans[-1][1] = plan.data_end + len(tail)
    plan.spans = [tuple(span) for span in plan.spans]
    plan.first = plan.frames[0][1] - plan.frames[0][0]
    plan.samples = sum(audio[:plan.fit])//block
    plan.largest, plan.largest_audio = max(sizes[:plan.fit], default=0), max(audio[:plan.fit], default=0)
    return plan


def chunk(payload: bytes) -> bytes:
    """A frame as the ring's writer frames it: fourcc, little-endian size, payload, a pad byte to an even length"""
    return b"00dc" + struct.pack("<I", len(payload)) + payload + b"\0"*(len(payload) & 1)


def pcm_s16(samples) -> np.ndarray:
    """float samples → int16 of the same shape: clip(rint(float64(x)*32768), -32768, 32767), ties to even, NaN → 0"""
    scaled = np.rint(np.asarray(samples, np.float64)*32768.0)
    return np.clip(np.where(np.isnan(scaled), 0.0, scaled), -32768.0, 32767.0).astype("<i2")


def fps_fraction(fps) -> Fraction:
    """The rational rate/scale an AVI file states its fps as"""
    return Fraction(fps).limit_denominator(100000)


def audio_end(k: int, samplerate: int, rate: int, scale: int, total: int) -> int:
    """a(k): the sample frames in front of video frame k, of a clip of `total`"""
    return min(total, (k*samplerate*scale)//rate)


class SoundTrack:
    """The `auds` stream of an AVI export: the clip as the file holds it (`pcm`: (N, channels) int16) and its schedule"""

    def __init__(self, samples, samplerate: int):
        samples = np.asarray(samples)
        if samples.ndim == 1:
            samples = samples[:, None]
        if samples.ndim != 2 or not 1 <= samples.shape[1] <= 65535 or int(samplerate) < 1:
            raise ValueError(f"a sound track is (n, channels) samples at a positive rate, not {samples.shape} at {samplerate}")
        self.pcm = np.ascontiguousarray(pcm_s16(samples))
        self.samplerate, self.channels, self.block = int(samplerate), samples.shape[1], 2*samples.shape[1]

    def end(self, k: int, rate: int, scale: int) -> int:
        return audio_end(k, self.samplerate, rate, scale, self.pcm.shape[0])

    def ends(self, frames: int, fps) -> np.ndarray:
        """uint64 [frames]: where, in `pcm`'s bytes, the chunk behind video frame k ends (the table of sfx_ring_side_track)"""
        fraction = fps_fraction(fps)
        return np.array([self.block*self.end(k + 1, fraction.numerator, fraction.denominator) for k in range(frames)], np.uint64)

    def chunk(self, k: int, rate: int, scale: int) -> bytes:
        return self.pcm[self.end(k, rate, scale):self.end(k + 1, rate, scale)].tobytes()


def audio_chunk(payload: bytes) -> bytes:
    """The `01wb` chunk of a non-empty share of the track, as the ring's writer frames it"""
    return b"01wb" + struct.pack("<I", len(payload)) + payload + b"\0"*(len(payload) & 1) if payload else b""


class AviWriter:
    """The file around the `00dc` chunks. `begin()` writes the headers through the descriptor; the chunks follow (from the ring's
    writer, or `add()`); `finish(sizes)` appends `idx1` and patches the frame count and the sizes. With a `track`, the `01wb` chunk of
    frame k follows its `00dc` chunk (the ring's writer has the schedule as a table: SoundTrack.ends). With `opendml` (the bytes a RIFF
    chunk may span) the file is OpenDML: `add()` (or the ring's writer: sfx_ring_segments) leaves a gap of 24 zero bytes in front of
    every frame that is a cut, and `finish(sizes)` derives the cuts from the sizes and the schedule, makes the gaps `RIFF AVIX LIST
    movi`, appends the `ix##` chunks in place of `idx1` and patches the headers with their super indexes."""

    def __init__(self, fileno: int, width: int, height: int, fps: float, limit: int = RIFF_LIMIT, track: Optional[SoundTrack] = None,
                 fourcc: bytes = b"MJPG", bit_count: int = 24, opendml: Optional[int] = None):
        self.fileno, self.width, self.height, self.limit, self.track = fileno, width, height, limit, track
        self.fourcc, self.bit_count = fourcc, bit_count                # of the video stream: strh's handler, strf's biCompression / biBitCount
        self.opendml = check_opendml(opendml)
        rate = fps_fraction(fps)
        self.rate, self.scale = rate.numerator, rate.denominator
        self.sizes: list[int] = []

    def audio_bytes(self, k: int) -> int:
        """Payload bytes of the audio chunk behind video frame k (0: none is written)"""
        if self.track is None:
            return 0
        return self.track.block*(self.track.end(k + 1, self.rate, self.scale) - self.track.end(k, self.rate, self.scale))

    def headers(self, frames: int, movi_bytes: int, riff_bytes: int, largest: int, largest_audio: int = 0, plan: Optional[Layout] = None) -> bytes:
        if self.opendml is not None:
            return self.opendml_headers(plan)
        pixels, track = self.width*self.height*3, self.track
        avih = struct.pack("<14I", round(1e6*self.scale/self.rate), 0, 0, 0x110 if track else 0x10, frames, 0, 2 if track else 1, largest,
                           self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", self.fourcc, 0, 0, 0, 0, self.scale, self.rate, 0, frames, largest, 0xffffffff, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, self.bit_count, self.fourcc, pixels, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        streams = b"LIST" + struct.pack("<I", len(strl)) + strl
        if track:
            strh = struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, track.samplerate, 0, track.end(frames, self.rate, self.scale),
                               largest_audio, 0xffffffff, track.block, 0, 0, 0, 0)
            strf = struct.pack("<HHIIHH", 1, track.channels, track.samplerate, track.samplerate*track.block, track.block, 16)
            strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
            streams += b"LIST" + struct.pack("<I", len(strl)) + strl
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + streams
        return (b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl +
                b"LIST" + struct.pack("<I", movi_bytes) + b"movi")

    def opendml_headers(self, plan: Optional[Layout] = None) -> bytes:
        """The OpenDML file's headers up to the first chunk: placeholders without a `plan`, the same bytes patched with one"""
        track, pixels = self.track, self.width*self.height*3
        first, frames, largest, largest_audio, samples = (plan.first, plan.fit, plan.largest, plan.largest_audio, plan.samples) if plan else (0, 0, 0, 0, 0)

        def super_index(stream: int) -> bytes:
            found = plan.supers[stream] if plan else []
            body = struct.pack("<HBBI4s12x", 4, 0, 0, len(found), (b"00dc", b"01wb")[stream])
            body += b"".join(struct.pack("<QII", *entry) for entry in found) + b"\0"*(16*(SUPER_ENTRIES - len(found)))
            return b"indx" + struct.pack("<I", len(body)) + body

        def stream_list(strh: bytes, strf: bytes, stream: int) -> bytes:
            strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf + super_index(stream)
            return b"LIST" + struct.pack("<I", len(strl)) + strl

        avih = struct.pack("<14I", round(1e6*self.scale/self.rate), 0, 0, 0x110 if track else 0x10, first, 0, 2 if track else 1, largest,
                           self.width, self.height, 0, 0, 0, 0)
        streams = stream_list(struct.pack("<4s4sIHHIIIIIIII4H", b"vids", self.fourcc, 0, 0, 0, 0, self.scale, self.rate, 0, frames, largest, 0xffffffff, 0,
                                          0, 0, self.width, self.height),
                              struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, self.bit_count, self.fourcc, pixels, 0, 0, 0, 0), 0)
        if track:
            streams += stream_list(struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, track.samplerate, 0, samples, largest_audio,
                                               0xffffffff, track.block, 0, 0, 0, 0),
                                   struct.pack("<HHIIHH", 1, track.channels, track.samplerate, track.samplerate*track.block, track.block, 16), 1)
        dmlh = struct.pack("<I", frames) + b"\0"*244
        odml = b"odml" + b"dmlh" + struct.pack("<I", len(dmlh)) + dmlh
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + streams + b"LIST" + struct.pack("<I", len(odml)) + odml
        head = b"RIFF" + struct.pack("<I", 0) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
        start = len(head) + 12
        riff, movi = (plan.spans[0][1] - 8, plan.spans[0][1] - (start - 4)) if plan else (0, 0)
        return head[:4] + struct.pack("<I", riff) + head[8:] + b"LIST" + struct.pack("<I", movi) + b"movi"

    def begin(self) -> None:
        self.start = len(self.headers(0, 0, 0, 0))                     # where the first chunk goes
        self.rule = Segments(self.start, self.opendml) if self.opendml is not None else None
        os.write(self.fileno, self.headers(0, 0, 0, 0))

    def add(self, payload: bytes) -> None:
        sound = audio_chunk(self.track.chunk(len(self.sizes), self.rate, self.scale)) if self.track else b""
        gap = b"\0"*GAP_BYTES if self.rule is not None and self.rule.cut(len(chunk(payload)) + len(sound)) else b""
        os.write(self.fileno, gap + chunk(payload) + sound)
        self.sizes.append(len(payload))

    def layout(self, sizes: Iterable[int], start: Optional[int] = None) -> Layout:
        """The OpenDML layout of these payload sizes with this writer's track and budget (no file is touched)"""
        sizes = list(sizes)
        start = len(self.opendml_headers()) if start is None else start
        audio = [self.audio_bytes(k) for k in range(len(sizes))] if self.track else None
        return opendml_layout(sizes, audio, start, self.opendml, self.track.block if self.track else 1)

    def finish_opendml(self, sizes: list) -> None:
        plan = self.layout(sizes, self.start)
        if any(end - begin - 8 > RIFF_LIMIT for begin, end in plan.spans):
            raise RuntimeError(f"an OpenDML RIFF chunk holds 4 GiB: a frame of {plan.largest} bytes and its segment's indexes pass that")
        os.ftruncate(self.fileno, plan.data_end)
        os.pwrite(self.fileno, plan.tail, plan.data_end)
        for (begin, end), movi in zip(plan.spans[1:], plan.movis[1:]):
            os.pwrite(self.fileno, b"RIFF" + struct.pack("<I", end - begin - 8) + b"AVIX" + b"LIST" + struct.pack("<I", end - movi) + b"movi", begin)
        os.pwrite(self.fileno, self.opendml_headers(plan), 0)
        os.lseek(self.fileno, 0, os.SEEK_END)
        if plan.fit < len(sizes):
            raise RuntimeError(f"an OpenDML file of {self.opendml}-byte segments holds {SUPER_ENTRIES} of them: closed at frame {plan.fit} of {len(sizes)}; "
                               f"a larger segment size (opendml=bytes, up to {SEGMENT_RANGE[1]}) holds the whole export")

    def finish(self, sizes: Iterable[int] | None = None) -> None:
        sizes = list(self.sizes if sizes is None else sizes)
        if self.opendml is not None:
            return self.finish_opendml(sizes)
        # RIFF's size field counts everything behind it: the headers less 8, the chunks, idx1's 8 + 16 per chunk (a frame's own and
        # that of the audio behind it: a frame fits with its audio or not at all)
        audio = [self.audio_bytes(k) for k in range(len(sizes))]
        fit, chunks, entries = 0, 0, 0
        for size, sound in zip(sizes, audio):
            more = 8 + size + (size & 1) + ((8 + sound + (sound & 1)) if sound else 0)
            if self.start - 8 + chunks + more + 8 + 16*(entries + 1 + bool(sound)) > self.limit:
                break
            fit, chunks, entries = fit + 1, chunks + more, entries + 1 + bool(sound)
        os.ftruncate(self.fileno, self.start + chunks)
        os.lseek(self.fileno, 0, os.SEEK_END)
        index, offset = bytearray(), 4                                  # offsets count from the `movi` fourcc
        for size, sound in zip(sizes[:fit], audio):
            index += struct.pack("<4sIII", b"00dc", 0x10, offset, size)
            offset += 8 + size + (size & 1)
            if sound:
                index += struct.pack("<4sIII", b"01wb", 0x10, offset, sound)
                offset += 8 + sound + (sound & 1)
        os.write(self.fileno, b"idx1" + struct.pack("<I", len(index)) + bytes(index))
        riff = self.start - 8 + chunks + 8 + len(index)
        os.pwrite(self.fileno, self.headers(fit, 4 + chunks, riff, max(sizes[:fit], default=0), max(audio[:fit], default=0)), 0)
        if fit < len(sizes):
            advice = "write '.mjpeg' (no container, no limit)" if self.fourcc == b"MJPG" else "take \"pipe\" (the frames back to back, no limit) or shorter clips"
            raise RuntimeError(f"an AVI 1.0 file holds 4 GiB: closed at frame {fit} of {len(sizes)}; {advice} for the whole export")
