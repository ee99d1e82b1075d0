"""
Containers of a Motion-JPEG export (`scene.main(output="clip.avi", pixel_format="mjpeg")`): the frames are encoded on the device
(csrc/jpeg_kernels.hpp) and arrive at the sink's file descriptor already framed by the read-out ring's writer thread — as bare JPEG
images back to back (`.mjpeg`, `.mjpg`, "pipe"), or as the `00dc` chunks of a RIFF AVI 1.0 file (`.avi`). `AviWriter` is the rest of
that file: the headers in front of the chunks, written with placeholders, and behind them the `idx1` index and the patched sizes.

One `vids` stream, fourcc `MJPG` — or `MPNG` (`pixel_format="png"`: every `00dc` chunk a complete PNG file made by csrc/png_kernels.hpp; the
same file otherwise, sound track included; ffmpeg and VLC map that fourcc to their PNG decoders). AVI 1.0 holds 4 GiB: an export that
would pass it is closed, valid, at the last frame that fits and raises (OpenDML is not written; `.mjpeg` has no such limit).

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
    frame k follows its `00dc` chunk (the ring's writer has the schedule as a table: SoundTrack.ends)."""

    def __init__(self, fileno: int, width: int, height: int, fps: float, limit: int = RIFF_LIMIT, track: Optional[SoundTrack] = None,
                 fourcc: bytes = b"MJPG", bit_count: int = 24):
        self.fileno, self.width, self.height, self.limit, self.track = fileno, width, height, limit, track
        self.fourcc, self.bit_count = fourcc, bit_count                # of the video stream: strh's handler, strf's biCompression / biBitCount
        rate = fps_fraction(fps)
        self.rate, self.scale = rate.numerator, rate.denominator
        self.sizes: list[int] = []

    def audio_bytes(self, k: int) -> int:
        """Payload bytes of the audio chunk behind video frame k (0: none is written)"""
        if self.track is None:
            return 0
        return self.track.block*(self.track.end(k + 1, self.rate, self.scale) - self.track.end(k, self.rate, self.scale))

    def headers(self, frames: int, movi_bytes: int, riff_bytes: int, largest: int, largest_audio: int = 0) -> bytes:
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

    def begin(self) -> None:
        self.start = len(self.headers(0, 0, 0, 0))                     # where the first chunk goes
        os.write(self.fileno, self.headers(0, 0, 0, 0))

    def add(self, payload: bytes) -> None:
        sound = audio_chunk(self.track.chunk(len(self.sizes), self.rate, self.scale)) if self.track else b""
        os.write(self.fileno, chunk(payload) + sound)
        self.sizes.append(len(payload))

    def finish(self, sizes: Iterable[int] | None = None) -> None:
        sizes = list(self.sizes if sizes is None else sizes)
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
