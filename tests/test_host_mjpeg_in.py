"""
Motion-JPEG sources on the host (shaderflow_amd/mjpegsource.py, tests/jpeg_decode_ref.py): the containers read back what mjpeg.py
wrote, the header parser's refusals name their field, the staged frame says what the stream says, the float64 restatement of the
decode against libjpeg's pixels (stored by tests/golden/make_golden_jpeg_streams.py), and how many samples sit near a rounding tie.
"""
from __future__ import annotations

import hashlib
import json
import os
import struct
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpeg_decode_ref as D  # noqa: E402
import jpeg_ref as J  # noqa: E402

from shaderflow_amd import mjpegsource as M  # noqa: E402
from shaderflow_amd.mjpeg import AviWriter  # noqa: E402

GOLDEN = Path(__file__).resolve().parent/"golden"/"jpeg_streams.npz"
# tests/golden/make_golden_staged.py: every stream's staged frame as `stage` wrote it before it filled the `STAGED` record, and the
# Annex K Huffman tables as the device library's encoder writes them into its header
STAGED_GOLDEN = json.loads((Path(__file__).resolve().parent/"golden"/"staged_sha256.json").read_text())
# the largest difference between the restatement and libjpeg's pixels (Pillow 12.2) on each stored stream, measured with this file's
# restatement; the check is deterministic, so it has no margin
PILLOW_GAP = 3


def streams() -> dict:
    data = np.load(GOLDEN)
    return {name[:-7]: (data[name].tobytes(), data[name[:-7] + ".pillow"]) for name in data.files if name.endswith(".stream")}


STREAMS = streams()


def clip(count=5, width=48, height=32):
    return [J.encode(J.picture("noise", width, height, seed), 90) for seed in range(count)]


def write_avi(path, frames, fps=30.0, width=48, height=32):
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        writer = AviWriter(fd, width, height, fps)
        writer.begin()
        for frame in frames:
            writer.add(frame)
        writer.finish()
    finally:
        os.close(fd)


# ---- containers ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fps", [30.0, 29.97, 12.5])
def test_the_avi_reader_returns_what_the_writer_wrote(tmp_path, fps):
    frames = clip() + [J.encode(J.picture("gradient", 48, 32), 50)]            # sizes of both parities
    assert {len(frame) & 1 for frame in frames} == {0, 1}
    write_avi(tmp_path/"clip.avi", frames, fps)
    reader = M.AviReader(tmp_path/"clip.avi")
    assert (reader.width, reader.height, reader.sampling, reader.components) == (48, 32, (2, 2), 3)
    assert abs(reader.fps - fps) < 1e-4 and len(reader) == len(frames) and reader.largest == max(map(len, frames))
    assert [size for _, size in reader.index] == [len(frame) for frame in frames]
    assert list(reader) == frames


def test_the_avi_reader_walks_movi_without_an_index_and_skips_other_chunks(tmp_path):
    frames = clip(3)
    write_avi(tmp_path/"clip.avi", frames)
    raw = (tmp_path/"clip.avi").read_bytes()
    at = raw.index(b"idx1")
    movi = raw.index(b"movi")
    audio = b"01wb" + struct.pack("<I", 3) + b"abc\0" + b"JUNK" + struct.pack("<I", 2) + b"zz"
    body = raw[:movi + 4] + audio + raw[movi + 4:at]
    body = body[:movi - 4] + struct.pack("<I", len(body) - movi) + body[movi:]
    body = body[:4] + struct.pack("<I", len(body) - 8) + body[8:]
    (tmp_path/"walk.avi").write_bytes(body)
    assert list(M.AviReader(tmp_path/"walk.avi")) == frames


def test_an_avi_of_another_codec_is_not_ours_and_avix_warns(tmp_path):
    write_avi(tmp_path/"clip.avi", clip(2))
    raw = (tmp_path/"clip.avi").read_bytes()
    (tmp_path/"other.avi").write_bytes(raw.replace(b"MJPG", b"H264"))
    with pytest.raises(LookupError, match="MJPG"):
        M.AviReader(tmp_path/"other.avi")
    (tmp_path/"long.avi").write_bytes(raw + b"RIFF" + struct.pack("<I", 4) + b"AVIX" + b"\0"*16)
    with pytest.warns(UserWarning, match="AVIX"):
        assert len(M.AviReader(tmp_path/"long.avi")) == 2
    (tmp_path/"not.avi").write_bytes(b"RIFFxxxxWAVE")
    with pytest.raises(ValueError, match="RIFF AVI"):
        M.AviReader(tmp_path/"not.avi")


def test_the_raw_splitter(tmp_path):
    frames = [STREAMS[name][0] for name in ("wide_420", "no_dht_420", "wide_420")] + clip(2)     # restart markers inside, DHT or none
    (tmp_path/"clip.mjpeg").write_bytes(b"".join(frames))
    reader = M.RawReader(tmp_path/"clip.mjpeg", fps=25)
    assert list(reader) == frames and reader.fps == 25.0 and reader.largest == max(map(len, frames))
    (tmp_path/"cut.mjpg").write_bytes(b"".join(frames)[:-7])                                    # a truncated last image ends the clip
    assert list(M.RawReader(tmp_path/"cut.mjpg", fps=25)) == frames[:-1]
    with pytest.raises(ValueError, match="fps="):
        M.RawReader(tmp_path/"clip.mjpeg", fps=None)
    (tmp_path/"junk.mjpeg").write_bytes(frames[0] + b"hello")
    with pytest.raises(ValueError, match="FF D8"):
        M.RawReader(tmp_path/"junk.mjpeg", fps=25)


# ---- the header parser ---------------------------------------------------------------------------------------------------------------

def patched(stream: bytes, marker: int, edit) -> bytes:
    """`stream` with the body of its first `marker` segment replaced by edit(body) (or the marker itself by edit's (marker, body))"""
    pos = 2
    while True:
        found, length = stream[pos + 1], struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        if found == marker:
            result = edit(stream[pos + 4:pos + 2 + length])
            new_marker, body = result if isinstance(result, tuple) else (marker, result)
            return stream[:pos] + bytes([0xff, new_marker]) + struct.pack(">H", len(body) + 2) + body + stream[pos + 2 + length:]
        pos += 2 + length


BASE = J.encode(J.picture("noise", 48, 32, 0), 90)


def sof(edit):
    return patched(BASE, 0xc0, lambda body: bytes(edit(bytearray(body))))


def with_bytes(body, changes):
    for at, value in changes.items():
        body[at] = value
    return body


REFUSALS = {
    "progressive": (patched(BASE, 0xc0, lambda body: (0xc2, body)), "SOF2"),
    "extended": (patched(BASE, 0xc0, lambda body: (0xc1, body)), "SOF1"),
    "arithmetic": (patched(BASE, 0xc0, lambda body: (0xc9, body)), "SOF9"),
    "twelve-bit": (sof(lambda body: with_bytes(body, {0: 12})), "precision 12"),
    "sixteen-bit-dqt": (patched(BASE, 0xdb, lambda body: bytes([0x10 | body[0]]) + body[1:]), "DQT with 16-bit"),
    "four-components": (patched(BASE, 0xc0, lambda body: body[:5] + bytes([4]) + body[6:] + bytes([4, 0x11, 1])), "4 components"),
    "sampling-1x2": (sof(lambda body: with_bytes(body, {7: 0x12})), "sampling factors"),
    "sampling-4x1": (sof(lambda body: with_bytes(body, {7: 0x41})), "sampling factors"),
    "chroma-2x1": (sof(lambda body: with_bytes(body, {10: 0x21})), "sampling factors"),
    "non-interleaved": (patched(BASE, 0xda, lambda body: bytes([1]) + body[1:3] + body[-3:]), "non-interleaved"),
    "spectral-selection": (patched(BASE, 0xda, lambda body: body[:-3] + bytes([0, 5, 0])), "spectral selection"),
    "no-soi": (b"\x00\x00" + BASE[2:], "SOI"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_every_refusal_names_its_field(case):
    stream, word = REFUSALS[case]
    with pytest.raises(ValueError, match=word):
        M.parse_header(stream)


def test_two_fields_in_one_chunk_and_another_geometry_are_refused():
    view = np.zeros(1 << 16, np.uint8)
    header = M.parse_header(BASE)
    assert M.stage(BASE, header, view) > M.FRAME_FIXED
    with pytest.raises(ValueError, match="two fields"):
        M.stage(BASE + BASE, header, view)
    with pytest.raises(ValueError, match="first frame"):
        M.stage(STREAMS["mid_420"][0], header, view)
    with pytest.raises(ValueError, match="slots hold"):
        M.stage(BASE, header, view[:2000])


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_the_staged_frame_says_what_the_stream_says(name):
    stream = STREAMS[name][0]
    info = J.decode(D.with_tables(stream))
    header = M.parse_header(stream)
    assert (header.width, header.height) == (info["width"], info["height"]) and header.restart_interval == info["restart_interval"]
    view = np.full(M.capacity_for(header, len(stream)), 0xaa, np.uint8)
    total = M.stage(stream, header, view)
    words = view[:24].view("<u4")
    mcus = info["coefficients"].shape[0]*info["coefficients"].shape[1]
    restart = info["restart_interval"] or mcus
    assert words[0] == M.FRAME_MAGIC and words[2] == restart and words[3] == -(-mcus//restart) and words[5] == header.components
    assert total == words[4] + words[1] and words[4] % 16 == 0
    scan = view[words[4]:total].tobytes()
    assert stream[header.scan_start:header.scan_start + len(scan)] == scan and stream[header.scan_start + len(scan):][:2] == b"\xff\xd9"
    offsets = view[M.FRAME_FIXED:M.FRAME_FIXED + 4*words[3]].view("<u4")
    assert offsets[0] == 0 and len(info["restart_markers"]) == words[3] - 1
    for k in range(1, words[3]):
        assert scan[offsets[k] - 2:offsets[k]] == bytes([0xff, 0xd0 + info["restart_markers"][k - 1]])
    for (kind, table), (bits, values) in info["tables"].items():
        base = 320 + 272*(2*kind + table)
        assert list(view[base:base + 16]) == bits and list(view[base + 16:base + 16 + len(values)]) == values
    for table, quant in info["quant"].items():
        assert np.array_equal(view[64 + 64*table:128 + 64*table][np.argsort(J.ZIGZAG)], quant)


def test_the_staged_record_mirrors_the_header_struct():
    fields = M.STAGED.fields
    assert M.STAGED.itemsize == 1536 == M.FRAME_FIXED
    assert [fields[name][1] for name in ("tq", "td", "ta", "quant", "huffman")] == [24, 28, 32, 64, 320]
    assert [fields[name][1] for name in ("magic", "scan_bytes", "restart", "intervals", "scan_offset", "components")] == [0, 4, 8, 12, 16, 20]
    assert M.STAGED["huffman"].subdtype[0].itemsize == 16 + 256 and sorted(M.STATUS_BITS) == [1, 2, 4, 8, 16]


def test_every_stream_has_a_recorded_staged_frame():
    assert sorted(STAGED_GOLDEN["staged"]) == sorted(STREAMS)


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_the_staged_frame_is_byte_for_byte_the_recorded_one(name):
    stream = STREAMS[name][0]
    header = M.parse_header(stream)
    view = np.full(M.capacity_for(header, len(stream)), 0xaa, np.uint8)
    total = M.stage(stream, header, view)
    assert hashlib.sha256(view[:total].tobytes()).hexdigest() == STAGED_GOLDEN["staged"][name]


def test_annex_k_is_the_device_library_s():
    recorded = {(int(key[0]), int(key[1])): (bytes.fromhex(bits), bytes.fromhex(values)) for key, (bits, values) in STAGED_GOLDEN["annex_k"].items()}
    assert recorded == M.ANNEX_K


# ---- the restatement -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(STREAMS))
def test_the_restatement_against_libjpeg(name):
    stream, pillow = STREAMS[name]
    info, rgb = D.pictures(stream)
    gap = np.abs(rgb.astype(np.int32) - pillow.astype(np.int32))
    print(f"{name}: max |restatement - libjpeg| = {gap.max()}, mean {gap.mean():.4f}")
    assert rgb.shape == pillow.shape and gap.max() <= PILLOW_GAP


def test_the_largest_gap_is_reached():
    assert max(int(np.abs(D.pictures(stream)[1].astype(np.int32) - pillow).max()) for stream, pillow in STREAMS.values()) == PILLOW_GAP


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_few_samples_sit_near_a_tie(name):
    share = float((D.tie_distance(D.decode(STREAMS[name][0])["samples"]) < 1e-3).mean())
    print(f"{name}: {share*100:.3f} % of the samples within 1e-3 of a tie")
    assert share <= 0.01


def test_our_own_streams_hold_the_hard_codes():
    extremes, sparse = {}, {}
    J.encode(J.picture("extremes", 48, 32, 0), 100, extremes)
    J.encode(J.picture("sparse", 40, 24, 0), 90, sparse)
    assert extremes["dc_size"] == 11 and sparse["zrl"] > 0
    assert J.encode(J.picture("extremes", 48, 32, 0), 100) == STREAMS["own_extremes"][0]


def test_slot_count_works_from_the_capacity():
    from shaderflow_amd.videosequence import SLOTS_MAX, slot_count
    header = M.JpegHeader(3840, 2160, 3, (2, 2), 240, 0)
    assert slot_count(M.capacity_for(header, 665_000)) == SLOTS_MAX and slot_count(3840*2160*3) == 10


def test_a_short_segment_is_refused_by_name_and_a_large_app_segment_is_walked(tmp_path):
    for marker, word in ((0xc0, "SOF0"), (0xda, "SOS"), (0xdd, "DRI")):
        stream = STREAMS["wide_420"][0] if marker == 0xdd else BASE
        with pytest.raises(ValueError, match=word):
            M.parse_header(patched(stream, marker, lambda body: body[:1]))
    # an image with 150 KB of APP2 segments (an ICC profile's worth) in front of its tables is split like any other
    large = BASE[:2] + (b"\xff\xe2" + struct.pack(">H", 50002) + b"\x5a"*50000)*3 + BASE[2:]
    (tmp_path/"clip.mjpeg").write_bytes(large + BASE)
    assert list(M.RawReader(tmp_path/"clip.mjpeg", fps=25)) == [large, BASE]


def test_a_dropped_frame_repeats_the_picture_in_front_of_it_and_the_file_is_closed(tmp_path):
    frames = clip(3)
    write_avi(tmp_path/"clip.avi", frames[:1] + [b""] + frames[1:] + [b""])
    reader = M.AviReader(tmp_path/"clip.avi")
    want = [frames[0], frames[0], frames[1], frames[2], frames[2]]
    assert len(reader) == 5 and list(reader) == want and reader.file.closed
    raw = (tmp_path/"clip.avi").read_bytes()                             # the same through the walk over movi
    (tmp_path/"walk.avi").write_bytes(raw.replace(b"idx1", b"JUNK"))
    walked = M.AviReader(tmp_path/"walk.avi")
    assert list(walked) == want
    opened = M.AviReader(tmp_path/"clip.avi")
    opened.close()
    assert opened.file.closed and next(opened, None) is None
