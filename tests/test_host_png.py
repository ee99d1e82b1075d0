"""
The PNG stream of csrc/png_kernels.hpp as tests/png_ref.py restates it, held against independent implementations on the CPU: Pillow
decodes every picture to exactly the source, zlib inflates the IDAT data to exactly the filtered stream and agrees on every CRC, the
size of every stripe is held against zlib's own Z_RLE coder, the code lengths are complete and within their limits, and the AVI
writer states MPNG (tests/avi_ref.py takes the file apart).
"""
import io
import os
import struct
import zlib

import numpy as np
import pytest

from shaderflow_amd import mjpeg
from tests import avi_ref as A
from tests import png_ref as P

CASES = [(w, h, kind) for w, h in P.SHAPES for kind in P.KINDS]
# A stripe's header writes 316 lengths without repeat symbols: 14 + 3 + 19*3 + 316*7 bits at the most, 3 of them BFINAL / BTYPE
HEADER_ALLOWANCE = 284
_encoded: dict = {}


def encoded(case):
    """(picture, the restatement's PNG file, its stats), made once per case"""
    if case not in _encoded:
        w, h, kind = case
        picture = P.picture(kind, w, h, seed=w*h)
        picture.setflags(write=False)
        stats: dict = {}
        _encoded[case] = (picture, P.encode(picture, stats), stats)
    return _encoded[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_pillow_and_zlib_read_the_stream(case):
    Image = pytest.importorskip("PIL.Image")
    picture, stream, _ = encoded(case)
    w, h, _ = case
    image = Image.open(io.BytesIO(stream))
    image.load()
    assert image.mode == "RGB" and np.array_equal(np.asarray(image), picture)
    found, end = P.chunks(stream)
    assert end == len(stream) <= P.capacity(w, h)
    assert [kind for kind, _, _ in found] == [b"IHDR"] + [b"IDAT"]*((h + 7)//8) + [b"IEND"]
    assert found[0][1] == struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
    for kind, data, crc in found:
        assert zlib.crc32(kind + data) == crc
    filtered, _ = P.filter_rows(picture)
    data = b"".join(data for kind, data, _ in found if kind == b"IDAT")
    assert data[:2] == b"\x78\x01" and zlib.decompress(data) == filtered.tobytes()
    assert P.adler32(filtered.tobytes()) == zlib.adler32(filtered.tobytes())
    for data in [data for kind, data, _ in found if kind == b"IDAT"][:-1]:
        assert data[-4:] == b"\x00\x00\xff\xff"


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_every_stripe_is_held_against_zlibs_rle_coder(case):
    """Each stripe's filtered bytes through zlib's Z_RLE deflate and a sync flush is the reference: the restatement's stripe may exceed
    it by the header written without repeat symbols and by nothing else (the length limiter did not run on any of these pictures:
    no symbol of an unlimited code is deeper than 15, asserted below, so it loses nothing here)."""
    assert hasattr(zlib, "Z_RLE"), "the local zlib has no Z_RLE strategy"
    picture, _, stats = encoded(case)
    filtered, _ = P.filter_rows(picture)
    payloads = P.idat_payloads(filtered)
    stripes = P.stripes_of(filtered)
    for k, (stripe, payload) in enumerate(zip(stripes, payloads)):
        coder = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        reference = coder.compress(stripe) + coder.flush(zlib.Z_SYNC_FLUSH)
        mine = len(payload) - (2 if k == 0 else 0) - (4 if k == len(stripes) - 1 else 0)
        print(f"{case} stripe {k}: {mine} bytes, zlib {len(reference)}, {'fixed' if stats['fixed'][k] else 'dynamic'}")
        assert mine <= len(reference) + HEADER_ALLOWANCE
        assert mine <= (9*len(stripe) + 7)//8 + 16
        counts = P.histogram(P.parse(stripe))
        assert P.code_lengths(counts[:P.LITERALS], 64).max() <= 15, "the limiter ran: its loss has to be measured"


def test_the_pictures_cover_every_filter_both_branches_and_long_runs():
    filters, branches, longest = set(), set(), 0
    for case in CASES:
        _, _, stats = encoded(case)
        filters |= set(stats["filters"])
        branches |= set(stats["fixed"])
        longest = max(longest, max(stats["longest_match"]))
    assert filters == {0, 1, 2, 3, 4} and branches == {False, True} and longest == 258
    zeros = P.parse(bytes(8*(3*344 + 1)))
    assert zeros[0] == ("literal", 0) and [v for _, v in zeros[1:]] == [258]*32 + [8*1033 - 1 - 32*258]   # a run longer than 258, across a flush


def test_the_parse_is_zlibs():
    """literal / match boundaries: a run of n equal bytes is one literal and matches of 258, then the rest as a match (3 and more) or literals"""
    for n in (1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 517, 520):
        tokens = P.parse(b"\x07"*n)
        assert sum(v if k == "match" else 1 for k, v in tokens) == n
        rest = (n - 1) % 258
        tail = [("match", rest)] if rest >= 3 else [("literal", 7)]*rest
        assert tokens == [("literal", 7)] + [("match", 258)]*((n - 1)//258) + tail, n
    assert P.parse(b"abbbbc") == [("literal", 97), ("literal", 98), ("match", 3), ("literal", 99)]
    assert [P.length_symbol(v) for v in (3, 10, 11, 12, 13, 18, 19, 257, 258)] == [
        (257, 0, 0), (264, 0, 0), (265, 1, 0), (265, 1, 1), (266, 1, 0), (268, 1, 1), (269, 2, 0), (284, 5, 30), (285, 0, 0)]


@pytest.mark.parametrize("name", ["fibonacci", "one-symbol", "no-match", "flat"])
def test_code_lengths_are_complete_and_limited(name):
    counts = P.histograms()[name]
    lengths, fixed, meta = P.tables(counts)
    for part, limit in ((lengths[:P.LITERALS], 15), (lengths[P.LITERALS:], 15), (meta, 7)):
        assert sum(2.0**-int(v) for v in part if v) == 1.0 and part.max() <= limit and (part > 0).sum() >= 2
    assert all(lengths[s] > 0 for s in range(P.SYMBOLS) if counts[s])
    if name == "fibonacci":
        assert P.code_lengths(counts[:P.LITERALS], 64).max() == 23, "unlimited, the code is 23 deep: the limiter has to run"
    if name == "one-symbol":
        assert list(np.flatnonzero(lengths)) == [0, 256, 286, 287] and fixed
    if name == "no-match":
        assert list(lengths[P.LITERALS:]) == [1, 1] + [0]*28
    codes = P.canonical(lengths[:P.LITERALS])
    used = sorted((int(lengths[s]), format(codes[s], f"0{int(lengths[s])}b")[::-1]) for s in range(P.LITERALS) if lengths[s])
    for (_, a), (_, b) in zip(used, used[1:]):
        assert not b.startswith(a), "prefix-free"


def test_the_avi_writer_states_mpng(tmp_path):
    """The file around the PNG payloads: strf says MPNG / 24, the frames are the payloads, idx1 lists them; with a track the schedule
    and the second stream are mjpeg's. The defaults stay MJPG (tests/test_host_avi_audio.py holds those headers)."""
    pictures = [P.picture(kind, 17, 8, seed=3) for kind in ("horizontal", "noise", "diagonal")]
    payloads = [P.encode(picture) for picture in pictures]
    samples = np.sin(np.arange(4410)[:, None]*np.array([0.01, 0.013]))*0.5
    for track in (None, mjpeg.SoundTrack(samples, 44100)):
        path = tmp_path/f"clip{0 if track is None else 1}.avi"
        with open(path, "wb", buffering=0) as file:
            writer = mjpeg.AviWriter(file.fileno(), 17, 8, 30.0, track=track, fourcc=b"MPNG", bit_count=24)
            writer.begin()
            for payload in payloads:
                writer.add(payload)
            writer.finish()
        avi = A.parse(path.read_bytes())
        assert A.video(avi) == payloads
        picture = avi["streams"][0]
        assert picture["strh"]["type"] == b"vids" and picture["strh"]["handler"] == b"MPNG" and picture["strh"]["length"] == 3
        assert struct.unpack("<IiiHH4sIiiII", picture["strf"]) == (40, 17, 8, 1, 24, b"MPNG", 17*8*3, 0, 0, 0, 0)
        if track is None:
            assert len(avi["streams"]) == 1 and A.order(avi) == [0, 0, 0]
        else:
            assert A.order(avi) == [4*(A.a(k + 1, 44100, 30, 4410) - A.a(k, 44100, 30, 4410)) for k in range(3)]
            assert A.audio(avi) == A.s16(samples).tobytes()[:4*A.a(3, 44100, 30, 4410)]
            assert avi["streams"][1]["strh"]["type"] == b"auds"
    default = mjpeg.AviWriter(os.open(os.devnull, os.O_WRONLY), 17, 8, 30.0)
    assert (default.fourcc, default.bit_count) == (b"MJPG", 24)
    os.close(default.fileno)
    with pytest.raises(ValueError, match=r"'png'.*\.avi"):
        mjpeg.container_of(".mp4", "png")
    with pytest.raises(ValueError, match=r"'png'.*\.avi"):
        mjpeg.container_of(".mjpeg", "png")
    assert mjpeg.container_of(".AVI", "png") == "avi" and mjpeg.container_of(".mjpeg") == "raw"
