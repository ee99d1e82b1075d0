"""
The Motion-JPEG export's host half, without a GPU: the float64 restatement of the stream (tests/jpeg_ref.py) against PIL in both
directions, the AVI writer, the validation of suffix and quality, and the inputs of the GPU tests (tests/test_gpu_mjpeg.py).
"""
import io
import os
import struct

import numpy as np
import pytest

from tests import jpeg_ref as J

PICTURES = [("gradient", 53, 37), ("noise", 40, 24), ("checker", 48, 32), ("sparse", 48, 48)]


def parse_avi(data: bytes) -> dict:
    """The structure of a RIFF AVI 1.0 file, every size and offset checked against the bytes: {"frames", "avih", "strh", "strf", "index"}"""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    out, pos = {"frames": []}, 12

    def chunks(start, end):
        pos = start
        while pos < end:
            fourcc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
            assert pos + 8 + size <= end, (fourcc, size, pos, end)
            yield fourcc, pos + 8, size
            pos += 8 + size + (size & 1)
        assert pos == end, (pos, end)
    for fourcc, body, size in chunks(12, len(data)):
        if fourcc == b"LIST" and data[body:body + 4] == b"hdrl":
            for inner, at, n in chunks(body + 4, body + size):
                if inner == b"avih":
                    out["avih"] = struct.unpack("<14I", data[at:at + n])
                elif inner == b"LIST":
                    assert data[at:at + 4] == b"strl"
                    for leaf, where, m in chunks(at + 4, at + n):
                        out[leaf.decode()] = data[where:where + m]
        elif fourcc == b"LIST":
            assert data[body:body + 4] == b"movi"
            out["movi"] = body
            for inner, at, n in chunks(body + 4, body + size):
                assert inner == b"00dc"
                out["frames"].append((at - 8 - body, data[at:at + n]))
        elif fourcc == b"idx1":
            out["index"] = [struct.unpack("<4sIII", data[body + 16*k:body + 16*k + 16]) for k in range(size//16)]
        else:
            raise AssertionError(fourcc)
    assert len(out["index"]) == len(out["frames"]) == out["avih"][4]
    for (fourcc, flags, offset, size), (at, payload) in zip(out["index"], out["frames"]):
        assert (fourcc, flags, offset, size) == (b"00dc", 0x10, at, len(payload))
    return out


@pytest.mark.parametrize("kind,w,h", PICTURES)
def test_reference_encoder_opens_in_pil(kind, w, h):
    Image = pytest.importorskip("PIL.Image")
    picture = J.picture(kind, w, h, seed=1)
    for quality in (25, 90, 100):
        stream = J.encode(picture, quality)
        image = Image.open(io.BytesIO(stream))
        image.load()
        assert image.size == (w, h) and image.mode == "RGB" and image.format == "JPEG"
        decoded = J.decode(stream)
        assert np.array_equal(decoded["coefficients"], J.coefficients(picture, quality))
        assert decoded["sampling"] == [(2, 2), (1, 1), (1, 1)] and decoded["restart_interval"] == (w + 15)//16
        assert all(np.array_equal(decoded["quant"][k], J.quant_tables(quality)[k]) for k in (0, 1))


@pytest.mark.parametrize("kind,w,h", PICTURES)
def test_reference_decoder_recovers_pil_coefficients(kind, w, h):
    """A baseline 4:2:0 JPEG with restart intervals that PIL wrote (the standard's Huffman tables): its coefficients, coded again with the
    file's own header and interval, are the file byte for byte — the decoder lost nothing and invented nothing"""
    Image = pytest.importorskip("PIL.Image")
    buffer = io.BytesIO()
    Image.fromarray(J.picture(kind, w, h, seed=2)).save(buffer, "JPEG", quality=85, subsampling=2, restart_marker_blocks=3)
    data = buffer.getvalue()
    decoded = J.decode(data)
    assert decoded["restart_interval"] == 3 and decoded["sampling"] == [(2, 2), (1, 1), (1, 1)] and (decoded["width"], decoded["height"]) == (w, h)
    assert decoded["tables"][(1, 0)] == (list(J.AC_LUMINANCE[0]), list(J.AC_LUMINANCE[1]))
    assert decoded["tables"][(1, 1)] == (list(J.AC_CHROMINANCE[0]), list(J.AC_CHROMINANCE[1]))
    scan = data.index(b"\xff\xda")
    prefix = data[:scan + 2 + struct.unpack(">H", data[scan + 2:scan + 4])[0]]
    assert J.encode_coefficients(decoded["coefficients"], w, h, 85, prefix=prefix, interval=3) == data
    assert decoded["coefficients"][:, :, :4].any()


def test_quality_scales_the_annex_k_tables():
    assert J.quant_tables(50)[0][:4].tolist() == [16, 11, 10, 16] and J.quant_tables(100)[1].tolist() == [1]*64
    assert J.quant_tables(90)[0][:4].tolist() == [3, 2, 2, 3] and J.quant_tables(1)[0].max() == 255
    assert J.quant_tables(25)[0][:3].tolist() == [32, 22, 20]
    for quality in (0, 101):
        with pytest.raises(ValueError):
            J.quant_tables(quality)


def test_avi_writer(tmp_path):
    """Canned payloads of odd and even length: RIFF, LIST and idx1 sizes and offsets hold; frame count and rate are in avih and strh"""
    from shaderflow_amd.mjpeg import AviWriter, chunk
    payloads = [bytes([k])*n for k, n in enumerate((1, 2, 7, 100, 33, 64))]
    for mode in ("add", "sizes"):
        path = tmp_path/f"{mode}.avi"
        with open(path, "wb", buffering=0) as file:
            writer = AviWriter(file.fileno(), 96, 64, 59.94)
            writer.begin()
            if mode == "add":
                for payload in payloads:
                    writer.add(payload)
                writer.finish()
            else:                                                       # the chunks arrive from elsewhere (the read-out ring's writer)
                os.write(file.fileno(), b"".join(chunk(p) for p in payloads))
                writer.finish([len(p) for p in payloads])
        avi = parse_avi(path.read_bytes())
        assert [payload for _, payload in avi["frames"]] == payloads
        assert avi["avih"][4] == 6 and avi["avih"][8:10] == (96, 64) and avi["avih"][0] == round(1e6*50/2997) and avi["avih"][3] & 0x10
        kind, handler, _, _, _, _, scale, rate, _, length = struct.unpack("<4s4sIHHIIIII", avi["strh"][:36])
        assert (kind, handler, length) == (b"vids", b"MJPG", 6) and rate/scale == pytest.approx(59.94)
        size, width, height, planes, bits, compression = struct.unpack("<IiiHH4s", avi["strf"][:20])
        assert (size, width, height, planes, bits, compression) == (40, 96, 64, 1, 24, b"MJPG")


def test_avi_writer_closes_a_valid_file_at_its_limit(tmp_path):
    from shaderflow_amd.mjpeg import AviWriter
    payloads = [bytes([k])*100 for k in range(6)]
    path = tmp_path/"limit.avi"
    with open(path, "wb", buffering=0) as file:
        writer = AviWriter(file.fileno(), 16, 16, 30.0)
        writer.begin()
        writer.limit = writer.start - 8 + 4*108 + 8 + 4*16 + 50             # room for four frames and their index, not five
        for payload in payloads:
            writer.add(payload)
        with pytest.raises(RuntimeError, match=r"\.mjpeg"):
            writer.finish()
    avi = parse_avi(path.read_bytes())
    assert [payload for _, payload in avi["frames"]] == payloads[:4] and len(path.read_bytes()) - 8 <= writer.limit


def test_suffix_and_quality_validation():
    from shaderflow_amd import mjpeg
    assert [mjpeg.container_of(s) for s in (".avi", ".AVI", ".mjpeg", ".mjpg")] == ["avi", "avi", "raw", "raw"]
    for suffix in (".mp4", ".rgb", ""):
        with pytest.raises(ValueError, match=r"\.avi.*\.mjpeg"):
            mjpeg.container_of(suffix)
    assert mjpeg.check_quality(1) == 1 and mjpeg.check_quality(100) == 100
    for quality in (0, 101, 90.0, "90", True, None):
        with pytest.raises(ValueError, match="jpeg_quality"):
            mjpeg.check_quality(quality)


def test_export_helper_validates_mjpeg_without_a_device(tmp_path):
    """pixel_format and suffix are judged before anything touches the GPU; no ffmpeg command is configured for mjpeg"""
    from types import SimpleNamespace

    from shaderflow_amd.exporting import ExportingHelper
    scene = SimpleNamespace(width=40, height=24, fps=30.0, runtime=1.0, ffmpeg=SimpleNamespace(time=0))
    helper = ExportingHelper(scene, pixel_format="mjpeg")
    helper.ffmpeg_sizes(40, 24)
    assert helper.mjpeg and helper.staged and not helper.planar and helper.frame_bytes == 64 + 48*32*3
    helper.ffmpeg_output(tmp_path/"clip.avi")
    assert (helper.kind, helper.container, helper.top_down) == ("path-mjpeg", "avi", False)
    helper = ExportingHelper(scene, pixel_format="mjpeg")
    helper.ffmpeg_output("pipe")
    assert helper.kind == "pipe"
    with pytest.raises(ValueError, match=r"\.avi.*\.mjpeg"):
        ExportingHelper(scene, pixel_format="mjpeg").ffmpeg_output(tmp_path/"clip.mp4")
    with pytest.raises(ValueError, match="jpeg_quality"):
        ExportingHelper(scene, pixel_format="mjpeg", jpeg_quality=0).ffmpeg_sizes(40, 24)
    with pytest.raises(ValueError, match="pixel_format 'nv12'.*'mjpeg'"):
        ExportingHelper(scene, pixel_format="nv12").ffmpeg_sizes(40, 24)


GPU_INPUTS = [(kind, w, h) for kind in ("gradient", "noise", "checker") for (w, h) in ((16, 16), (48, 32), (40, 24), (17, 9), (1040, 16))]


@pytest.mark.parametrize("kind,w,h", GPU_INPUTS)
def test_gpu_inputs_leave_at_most_one_percent_near_a_tie(kind, w, h):
    """The coefficient test compares exactly except within 1e-3 of a rounding tie: on its inputs that leaves out at most 1 %"""
    picture = J.picture(kind, w, h, seed=J.NOISE_SEEDS[(w, h)])
    for quality in (50, 90, 100):
        near = J.tie_distance(picture, quality) <= 1e-3
        assert near.mean() <= 0.01, (kind, w, h, quality, float(near.mean()))


def test_gpu_entropy_inputs_have_what_they_are_for():
    """An 11-bit DC difference and a stuffed byte; ZRL codes; the overflow case's size against its capacity"""
    stats: dict = {}
    stream = J.encode(J.picture("extremes", 64, 48, seed=5), 100, stats)
    assert stats["dc_size"] == 11 and b"\xff\x00" in stream[len(J.header(64, 48, 100)):]
    stats = {}
    J.encode(J.picture("sparse", 48, 48, seed=5), 25, stats)
    assert stats["zrl"] > 0
    assert len(J.encode(J.picture("noise", 16, 16, seed=5), 100)) > 1.25*768


def test_psnr_of_the_definition_beside_libjpeg():
    """The definition's PSNR against the source beside libjpeg's at the same tables and sampling: the CPU's number for the definition
    (integer colour coefficients, chroma from the mean of R, G, B), not a bound on the device. DESIGN.md §7b quotes these figures."""
    Image = pytest.importorskip("PIL.Image")
    for kind, w, h in (("gradient", 96, 64), ("noise", 96, 64), ("checker", 96, 64)):
        picture = J.picture(kind, w, h, seed=3)
        for quality in (75, 90):
            luma, chroma = J.quant_tables(quality)
            buffer = io.BytesIO()
            Image.fromarray(picture).save(buffer, "JPEG", qtables=[[int(v) for v in luma[J.ZIGZAG]], [int(v) for v in chroma[J.ZIGZAG]]], subsampling=2)
            theirs = J.psnr(np.asarray(Image.open(buffer).convert("RGB")), picture)
            ours = J.psnr(np.asarray(Image.open(io.BytesIO(J.encode(picture, quality))).convert("RGB")), picture)
            print(f"{kind} q{quality}: definition {ours:.2f} dB, libjpeg {theirs:.2f} dB, difference {ours - theirs:+.2f} dB")
            assert np.isfinite(ours) or kind == "checker"
