"""
A RIFF AVI 1.0 file with a Motion-JPEG stream and, optionally, a PCM stream beside it, taken apart with every size and offset checked
against the bytes (tests/test_host_mjpeg.py's parse_avi knows the single-stream file and asserts that it is one). Also the sound
track's definition restated with `fractions.Fraction`, for the tests to hold shaderflow_amd/mjpeg.py against.
"""
import struct
from fractions import Fraction

import numpy as np

STRH = "<4s4sIHHIIIIIIII4H"
STRH_FIELDS = ("type", "handler", "flags", "priority", "language", "initial_frames", "scale", "rate", "start", "length",
               "suggested_buffer", "quality", "sample_size", "left", "top", "right", "bottom")


def parse(data: bytes) -> dict:
    """{"avih": 14 ints, "streams": [{"strh": {field: value}, "strf": bytes}], "chunks": [(fourcc, offset from the movi fourcc, payload)],
    "index": [(fourcc, flags, offset, size)], "start": file offset of the first chunk}; idx1 is checked against the chunks found"""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    out = {"streams": [], "chunks": []}

    def chunks(start, end):
        pos = start
        while pos < end:
            fourcc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
            assert pos + 8 + size <= end, (fourcc, size, pos, end)
            if size & 1 and pos + 8 + size < end:
                assert data[pos + 8 + size] == 0, "the pad byte is zero"
            yield fourcc, pos + 8, size
            pos += 8 + size + (size & 1)
        assert pos == end, (pos, end)
    top = [fourcc if fourcc != b"LIST" else data[body:body + 4] for fourcc, body, _ in chunks(12, len(data))]
    assert top == [b"hdrl", b"movi", b"idx1"], top
    for fourcc, body, size in chunks(12, len(data)):
        if fourcc == b"LIST" and data[body:body + 4] == b"hdrl":
            inner = list(chunks(body + 4, body + size))
            assert [name for name, _, _ in inner] == [b"avih"] + [b"LIST"]*(len(inner) - 1)
            out["avih"] = struct.unpack("<14I", data[inner[0][1]:inner[0][1] + inner[0][2]])
            for _, at, n in inner[1:]:
                assert data[at:at + 4] == b"strl"
                leaves = list(chunks(at + 4, at + n))
                assert [name for name, _, _ in leaves] == [b"strh", b"strf"]
                (_, h_at, h_n), (_, f_at, f_n) = leaves
                assert h_n == struct.calcsize(STRH)
                out["streams"].append({"strh": dict(zip(STRH_FIELDS, struct.unpack(STRH, data[h_at:h_at + h_n]))), "strf": data[f_at:f_at + f_n]})
        elif fourcc == b"LIST":
            out["start"] = body + 4
            for inner, at, n in chunks(body + 4, body + size):
                out["chunks"].append((inner, at - 8 - body, data[at:at + n]))
        else:
            assert size % 16 == 0
            out["index"] = [struct.unpack("<4sIII", data[body + 16*k:body + 16*k + 16]) for k in range(size//16)]
    assert out["index"] == [(fourcc, 0x10, offset, len(payload)) for fourcc, offset, payload in out["chunks"]]
    assert len(out["streams"]) == out["avih"][6]
    return out


def video(avi: dict) -> list:
    return [payload for fourcc, _, payload in avi["chunks"] if fourcc == b"00dc"]


def audio(avi: dict) -> bytes:
    return b"".join(payload for fourcc, _, payload in avi["chunks"] if fourcc == b"01wb")


def order(avi: dict) -> list:
    """Per video frame, the bytes of the audio chunk behind it (0: none); asserts that nothing else is in `movi`, that no audio chunk is
    empty and that none stands anywhere but right behind a frame"""
    sizes = []
    for k, (fourcc, _, payload) in enumerate(avi["chunks"]):
        if fourcc == b"00dc":
            sizes.append(0)
        else:
            assert fourcc == b"01wb" and len(payload) > 0 and k > 0 and avi["chunks"][k - 1][0] == b"00dc", (k, fourcc, len(payload))
            sizes[-1] = len(payload)
    return sizes


def a(k: int, samplerate: int, fps, total: int) -> int:
    """Sample frames in front of video frame k: floor(k*samplerate/fps), at most the clip, in exact rational arithmetic"""
    return min(total, int(Fraction(k)*samplerate/Fraction(fps).limit_denominator(100000)//1))


def s16(samples) -> np.ndarray:
    """clip(rint(float64(x)*32768), -32768, 32767), ties to even, NaN → 0 — value by value, with Python's round()"""
    flat = [0 if x != x else round(max(-32768.0, min(32767.0, float(x)*32768.0))) for x in np.asarray(samples, np.float64).ravel()]
    return np.array(flat, "<i2").reshape(np.shape(samples))


def check_streams(avi: dict, width: int, height: int, fps, frames: int, channels: int, samplerate: int, sample_frames: int) -> None:
    """avih and both strl lists, field by field"""
    fraction = Fraction(fps).limit_denominator(100000)
    largest = max((len(p) for p in video(avi)), default=0)
    largest_audio = max(order(avi), default=0)
    assert avi["avih"] == (round(1e6/fraction), 0, 0, 0x110, frames, 0, 2, largest, width, height, 0, 0, 0, 0)
    picture, sound = avi["streams"]
    assert picture["strh"] == dict(type=b"vids", handler=b"MJPG", flags=0, priority=0, language=0, initial_frames=0, scale=fraction.denominator,
                                   rate=fraction.numerator, start=0, length=frames, suggested_buffer=largest, quality=0xffffffff, sample_size=0,
                                   left=0, top=0, right=width, bottom=height)
    assert struct.unpack("<IiiHH4sIiiII", picture["strf"]) == (40, width, height, 1, 24, b"MJPG", width*height*3, 0, 0, 0, 0)
    block = 2*channels
    assert sound["strh"] == dict(type=b"auds", handler=b"\0\0\0\0", flags=0, priority=0, language=0, initial_frames=0, scale=1, rate=samplerate,
                                 start=0, length=sample_frames, suggested_buffer=largest_audio, quality=0xffffffff, sample_size=block,
                                 left=0, top=0, right=0, bottom=0)
    assert len(sound["strf"]) == 16
    assert struct.unpack("<HHIIHH", sound["strf"]) == (1, channels, samplerate, samplerate*block, block, 16)
