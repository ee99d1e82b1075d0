"""
PNG sources on the host (shaderflow_amd/pngsource.py) and the plain-Python restatement of the device's decode (tests/png_decode_ref.py):
the restatement against zlib and Pillow on every case of the table the GPU tests share, the parser's refusals, the staged frame's
layout, the AVI reader on MPNG and MJPG files, and the rule that sends a frame down the segment path.
"""
from __future__ import annotations

import io
import os
import struct
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import png_decode_ref as D  # noqa: E402
import png_ref as P  # noqa: E402

from shaderflow_amd import pngsource as S  # noqa: E402

CASES = D.cases()


def inflated(stream: bytes) -> bytes:
    return zlib.decompress(b"".join(data for kind, data, _ in P.chunks(stream)[0] if kind == b"IDAT"))


def pillow_rgb(stream: bytes) -> np.ndarray:
    Image = pytest.importorskip("PIL.Image")
    return np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_restatement_is_zlib_and_pillow(name):
    case = CASES[name]
    for segments in case["paths"]:
        got = D.decode(case["stream"], segments=segments)
        assert got["status"] == 0
        assert got["filtered"] == inflated(case["stream"])
        assert np.array_equal(got["rgb"], pillow_rgb(case["stream"]))


@pytest.mark.parametrize("name", sorted(D.damaged()))
def test_the_restatement_names_the_damage(name):
    stream, bit = D.damaged()[name]
    assert D.decode(stream)["status"] == bit


def test_the_status_bits_are_the_headers():
    header = (Path(__file__).resolve().parents[1]/"include"/"shaderflow_hip.h").read_text()
    for name in ("BAD_BLOCK", "BAD_STORED", "BAD_LENGTHS", "BAD_CODE", "BAD_DISTANCE", "OUT_OF_BITS", "BAD_SIZE", "BAD_FILTER", "BAD_ADLER", "BAD_DESCRIPTOR"):
        assert f"SFX_PNG_{name} = {getattr(S, name)}" in header and getattr(S, name) == getattr(D, name)
        assert S.describe_status(getattr(S, name)) == S.STATUS_BITS[getattr(S, name)]
    assert f"SFX_PNG_FRAME_MAGIC = {S.FRAME_MAGIC:#x}" in header and S.FRAME_MAGIC != 0x444a4653
    assert S.describe_status(S.BAD_CODE | S.BAD_ADLER).count(";") == 1


def with_ihdr(**fields) -> bytes:
    values = dict(width=4, height=4, depth=8, colour=2, compression=0, method=0, interlace=0)
    values.update(fields)
    body = zlib.compress(bytes(4*13))
    return P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", *values.values())) + P.chunk(b"IDAT", body) + P.chunk(b"IEND", b"")


@pytest.mark.parametrize("fields, words", [
    (dict(depth=16), "bit depth 16"), (dict(depth=4), "bit depth 4"), (dict(colour=3), "colour type 3 (palette)"), (dict(colour=0), "colour type 0 (grey)"),
    (dict(colour=6), "colour type 6 (RGB with alpha)"), (dict(colour=4), "colour type 4"), (dict(compression=1), "compression method 1"),
    (dict(method=1), "filter method 1"), (dict(interlace=1), "interlace method 1 (Adam7)"), (dict(width=0), "width 0")])
def test_the_parser_refuses_by_ihdr_field(fields, words):
    with pytest.raises(ValueError, match=words.replace("(", r"\(").replace(")", r"\)")):
        S.parse_header(with_ihdr(**fields))
    assert S.parse_header(with_ihdr()).geometry == (4, 4)


def test_the_parser_walks_the_chunks():
    stream = CASES["own-37x21"]["stream"]
    header = S.parse_header(stream)
    assert (header.width, header.height, len(header.payloads), header.end) == (37, 21, 3, len(stream))
    assert [bytes(p) for p in header.payloads] == [data for kind, data, _ in P.chunks(stream)[0] if kind == b"IDAT"]
    # ancillary chunks are skipped, wherever they stand; CRCs are not looked at
    text = P.chunk(b"tEXt", b"Comment\0hello")
    extra = stream[:33] + text + P.chunk(b"gAMA", struct.pack(">I", 45455)) + stream[33:-12] + text + stream[-12:]
    assert [bytes(p) for p in S.parse_header(extra).payloads] == [bytes(p) for p in header.payloads]
    broken = bytearray(stream)
    broken[29] ^= 0xff                                                 # IHDR's CRC
    assert S.parse_header(bytes(broken)).geometry == (37, 21)
    with pytest.raises(ValueError, match="critical chunk b'FOOB'"):
        S.parse_header(stream[:33] + P.chunk(b"FOOB", b"") + stream[33:])
    with pytest.raises(ValueError, match="no signature"):
        S.parse_header(b"\xff\xd8" + stream)
    # truncation, anywhere: inside a chunk, between chunks, in front of IEND
    for cut in (20, 33, 40, len(stream) - 12, len(stream) - 1):
        with pytest.raises(ValueError, match="cut short"):
            S.parse_header(stream[:cut])
    with pytest.raises(ValueError, match="second picture"):
        S.parse_header(stream + stream)
    assert S.parse_header(stream + b"\0\0junk").end == len(stream)
    for bad in (b"\x78\x02", b"\x79\x01", b"\x88\x1c", b"\x78\x20"):   # the check bits, CM = 9, a 64 KiB window, FDICT
        with pytest.raises(ValueError, match="no valid zlib header"):
            S.parse_header(D.png(4, 4, [bad + zlib.compress(bytes(52))[2:]]))


@pytest.mark.parametrize("name", ["own-86x129", "pillow-0", "zlib-1x1", "flush-bytes-in-a-stored-block"])
def test_the_staged_frame_round_trips(name):
    stream = CASES[name]["stream"]
    header = S.parse_header(stream)
    view = np.full(S.capacity_for(header, len(stream)), 0xa5, np.uint8)
    total = S.stage(stream, header, view, "frame")
    width, height, payload, starts, adler = D.split(stream)
    fixed = view[:S.FRAME_FIXED].view(S.STAGED)[0]
    assert (fixed["magic"], fixed["width"], fixed["height"], fixed["segments"]) == (S.FRAME_MAGIC, width, height, len(starts))
    assert fixed["payload_offset"] % 16 == 0 and fixed["payload_offset"] == S.FRAME_FIXED + ((4*len(starts) + 15) & ~15)
    assert (fixed["payload_bytes"], fixed["adler"]) == (len(payload), adler) and total == fixed["payload_offset"] + len(payload) <= S.staged_bytes(header)
    assert view[S.FRAME_FIXED:S.FRAME_FIXED + 4*len(starts)].view("<u4").tolist() == starts
    assert not view[S.FRAME_FIXED + 4*len(starts):fixed["payload_offset"]].any()
    assert bytes(view[fixed["payload_offset"]:total]) == payload
    assert not view[total:total + 4].any() and (view[total + 4:] == 0xa5).all()
    # the payload inflates on its own, and its Adler-32 is the record's
    assert zlib.adler32(zlib.decompressobj(-15).decompress(payload)) == adler
    # another geometry than the clip's, and a slot that is too small
    with pytest.raises(ValueError, match="the clip's first frame has 3 x 3"):
        S.stage(stream, S.PngHeader(3, 3), view, "frame 7")
    with pytest.raises(ValueError, match="frame 7.*need a slot"):
        S.stage(stream, header, view[:total], "frame 7")


def write_avi(path, frames, width, height, fps, fourcc=b"MPNG", sound=None):
    from shaderflow_amd.mjpeg import AviWriter, SoundTrack
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        track = SoundTrack(sound, 8000) if sound is not None else None
        writer = AviWriter(fd, width, height, fps, track=track, fourcc=fourcc)
        writer.begin()
        for frame in frames:
            writer.add(frame)
        writer.finish()
    finally:
        os.close(fd)


@pytest.mark.parametrize("sound", [False, True])
def test_the_avi_reader_finds_mpng(sound, tmp_path):
    from shaderflow_amd import mjpegsource
    frames = [P.encode(D.mixed(37, 21, seed)) for seed in range(4)]
    pcm = np.sin(np.arange(8000*4//30 + 1)[:, None]*np.array([[0.05, 0.07]])).astype(np.float32) if sound else None
    write_avi(tmp_path/"clip.avi", frames, 37, 21, 30.0, sound=pcm)
    reader = S.AviReader(tmp_path/"clip.avi")
    assert (reader.width, reader.height, reader.fps, reader.format, reader.largest) == (37, 21, 30.0, "png", max(map(len, frames)))
    assert list(reader) == frames
    with pytest.raises(LookupError, match="MJPG"):
        mjpegsource.AviReader(tmp_path/"clip.avi")
    # MJPG files are found as before, and not by this reader; another codec is LookupError from both
    write_avi(tmp_path/"other.avi", frames, 37, 21, 30.0, fourcc=b"H264")
    for reader in (mjpegsource.AviReader, S.AviReader):
        with pytest.raises(LookupError):
            reader(tmp_path/"other.avi")


def test_the_avi_reader_still_finds_mjpg(tmp_path):
    import jpeg_ref as J
    from shaderflow_amd import mjpegsource
    frames = [J.encode(J.picture("noise", 48, 32, seed), 90) for seed in range(3)]
    write_avi(tmp_path/"clip.avi", frames, 48, 32, 25.0, fourcc=b"MJPG")
    reader = mjpegsource.AviReader(tmp_path/"clip.avi")
    assert (reader.width, reader.height, reader.fps, reader.format) == (48, 32, 25.0, "mjpeg") and list(reader) == frames
    with pytest.raises(LookupError, match="MPNG"):
        S.AviReader(tmp_path/"clip.avi")


def test_one_walk_opens_an_avi_for_either_codec(tmp_path):
    import jpeg_ref as J
    from shaderflow_amd import mjpegsource
    from shaderflow_amd.clips import AviClip
    pngs = [P.encode(D.mixed(37, 21, seed)) for seed in range(4)]
    jpegs = [J.encode(J.picture("noise", 48, 32, seed), 90) for seed in range(3)]
    write_avi(tmp_path/"jpeg.avi", jpegs, 48, 32, 25.0, fourcc=b"MJPG")
    write_avi(tmp_path/"png.avi", pngs, 37, 21, 30.0)
    write_avi(tmp_path/"other.avi", pngs, 37, 21, 30.0, fourcc=b"H264")
    codecs = (mjpegsource, S)
    clip = AviClip(tmp_path/"jpeg.avi", codecs)
    assert (clip.format, clip.width, clip.height, clip.fps, clip.sampling, clip.components) == ("mjpeg", 48, 32, 25.0, (2, 2), 3) and list(clip) == jpegs
    clip = AviClip(tmp_path/"png.avi", codecs)
    assert (clip.format, clip.width, clip.height, clip.fps, clip.largest) == ("png", 37, 21, 30.0, max(map(len, pngs))) and list(clip) == pngs
    assert not hasattr(clip, "sampling")
    descriptors = len(os.listdir("/proc/self/fd"))
    with pytest.raises(LookupError, match="MJPG.*MPNG"):
        AviClip(tmp_path/"other.avi", codecs)
    assert len(os.listdir("/proc/self/fd")) == descriptors
    # the failed open closed its file and its map: the path opens again, and may be written over
    with pytest.raises(LookupError, match="MPNG"):
        S.AviReader(tmp_path/"other.avi")
    write_avi(tmp_path/"other.avi", pngs, 37, 21, 30.0)
    assert list(AviClip(tmp_path/"other.avi", codecs)) == pngs


def test_the_rule_that_chooses_the_segment_path(monkeypatch):
    monkeypatch.delenv("SHADERFLOW_PNG_SEGMENTS", raising=False)
    for name, case in CASES.items():
        width, height, payload, starts, _ = D.split(case["stream"])
        assert S.segment_path(S.parse_header(case["stream"])) == D.segment_rule(payload, starts), name
    chosen = {name for name, case in CASES.items() if S.segment_path(S.parse_header(case["stream"]))}
    assert {"own-37x21", "own-86x129", "full-flush", "sync-flush", "flush-bytes-in-a-stored-block"} <= chosen
    assert not chosen & {"pillow-0", "pillow-9", "own-1x1", "own-7x1", "stored", "zlib-86x129"}
    # what the rule lets through and validation must catch: every case the device falls back on decodes invalid on its own here
    for name in D.FELL_BACK:
        got = D.decode(CASES[name]["stream"], segments=True)
        assert got["info"] == {"segments": len(D.split(CASES[name]["stream"])[3]), "parallel": 0, "fell_back": 1} and got["status"] == 0
    for name in D.PARALLEL:
        assert D.decode(CASES[name]["stream"])["info"]["parallel"] == 1
    monkeypatch.setenv("SHADERFLOW_PNG_SEGMENTS", "0")
    assert not S.segment_path(S.parse_header(CASES["own-37x21"]["stream"]))
    monkeypatch.setenv("SHADERFLOW_PNG_SEGMENTS", "1")
    assert S.segment_path(S.parse_header(CASES["pillow-9"]["stream"]))

