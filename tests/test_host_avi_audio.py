"""
The sound track of a Motion-JPEG AVI export, without a GPU: the two-stream file `mjpeg.AviWriter` writes, the schedule that shares the
clip out among the frames, the 16-bit quantisation, the 4 GiB accounting with audio in it, reading the track back
(`audio.reader.decode_audio`), and that a writer without a track writes what it always wrote. tests/avi_ref.py parses and restates.
"""
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

from shaderflow_amd import mjpeg
from tests import avi_ref as A

SIZES = (1, 2, 7, 100, 33, 64, 501)                                     # odd and even
PAYLOADS = [bytes([k + 1])*n for k, n in enumerate(SIZES)]
CASES = {"30-44100-stereo": (30, 44100, 2, 12000), "29.97-8000-mono": (Fraction(2997, 100), 8000, 1, 3000)}


def clip(total: int, channels: int, seed: int = 7) -> np.ndarray:
    return np.random.default_rng(seed).uniform(-1.1, 1.1, (total, channels)).astype(np.float32)


def write(path, fps, track, payloads=PAYLOADS, mode="add", limit=None, width=96, height=64):
    """The file, through `add()` or with the chunks arriving from elsewhere as the read-out ring's writer sends them"""
    with open(path, "wb", buffering=0) as file:
        writer = mjpeg.AviWriter(file.fileno(), width, height, fps, track=track, **({} if limit is None else {"limit": limit}))
        writer.begin()
        if mode == "add":
            for payload in payloads:
                writer.add(payload)
            writer.finish()
        else:
            for k, payload in enumerate(payloads):
                os.write(file.fileno(), mjpeg.chunk(payload) + (mjpeg.audio_chunk(track.chunk(k, writer.rate, writer.scale)) if track else b""))
            writer.finish([len(p) for p in payloads])
    return path.read_bytes()


@pytest.mark.parametrize("mode", ["add", "sizes"])
@pytest.mark.parametrize("case", list(CASES))
def test_the_file(case, mode, tmp_path):
    """Seven fake frames and a clip longer than they last: every RIFF and LIST size is exact and idx1 is the chunks found by walking
    (avi_ref.parse), avih and both strl lists hold field by field, `00dc` then `01wb` frame by frame, and the audio is the quantised
    clip up to a(7)"""
    fps, samplerate, channels, total = CASES[case]
    samples = clip(total, channels)
    avi = A.parse(write(tmp_path/"clip.avi", fps, mjpeg.SoundTrack(samples, samplerate), mode=mode))
    end = A.a(7, samplerate, fps, total)
    assert 0 < end < total
    A.check_streams(avi, 96, 64, fps, 7, channels, samplerate, end)
    assert A.video(avi) == PAYLOADS
    assert A.order(avi) == [2*channels*(A.a(k + 1, samplerate, fps, total) - A.a(k, samplerate, fps, total)) for k in range(7)]
    assert [fourcc for fourcc, _, _ in avi["chunks"]] == [b"00dc", b"01wb"]*7
    assert A.audio(avi) == mjpeg.pcm_s16(samples)[:end].tobytes() == A.s16(samples[:end]).tobytes()
    assert avi["streams"][1]["strh"]["length"] == end


@pytest.mark.parametrize("case", list(CASES))
def test_the_schedule_is_the_rational_one(case):
    fps, samplerate, channels, _ = CASES[case]
    total = 10**9
    track = mjpeg.SoundTrack(np.zeros((4, channels), np.float32), samplerate)
    fraction = Fraction(fps).limit_denominator(100000)
    assert mjpeg.fps_fraction(fps) == fraction == Fraction(fps)
    for k in range(1001):
        want = int(Fraction(k*samplerate)/fraction//1)
        assert mjpeg.audio_end(k, samplerate, fraction.numerator, fraction.denominator, total) == want == A.a(k, samplerate, fps, total)
        assert track.end(k, fraction.numerator, fraction.denominator) == min(4, want)
    ends = mjpeg.SoundTrack(np.zeros((50000, channels), np.float32), samplerate).ends(1000, fps)
    assert ends.dtype == np.uint64 and ends.tolist() == [2*channels*A.a(k + 1, samplerate, fps, 50000) for k in range(1000)]


def test_a_shorter_clip_simply_ends(tmp_path):
    """8 000 Hz at 29.97 fps gives frames 266.9 sample frames each: a clip of 700 ends inside the third, and frames 3 to 6 are `00dc` alone"""
    fps, samplerate = Fraction(2997, 100), 8000
    samples = clip(700, 1)
    avi = A.parse(write(tmp_path/"short.avi", fps, mjpeg.SoundTrack(samples, samplerate)))
    assert A.order(avi) == [2*266, 2*267, 2*167, 0, 0, 0, 0]
    assert [fourcc for fourcc, _, _ in avi["chunks"]] == [b"00dc", b"01wb"]*3 + [b"00dc"]*4
    assert A.audio(avi) == A.s16(samples).tobytes()
    A.check_streams(avi, 96, 64, fps, 7, 1, samplerate, 700)
    # and a clip that ends exactly where a frame does leaves no empty chunk behind the next
    avi = A.parse(write(tmp_path/"exact.avi", 30, mjpeg.SoundTrack(clip(2*1470, 2), 44100)))
    assert A.order(avi) == [4*1470, 4*1470, 0, 0, 0, 0, 0]


def test_a_longer_clip_is_cut_where_the_video_ends(tmp_path):
    samples = clip(44100, 2)
    avi = A.parse(write(tmp_path/"long.avi", 24, mjpeg.SoundTrack(samples, 44100)))
    assert A.a(7, 44100, 24, 44100) == 12862                           # 7*1837.5, rounded down
    assert A.audio(avi) == A.s16(samples[:12862]).tobytes() and avi["streams"][1]["strh"]["length"] == 12862
    assert A.order(avi) == [4*n for n in (1837, 1838, 1837, 1838, 1837, 1838, 1837)]


def test_pcm_s16_values():
    """±1 and beyond saturate (+1 has no 16-bit value), NaN is silence, zero of either sign is zero, and a tie goes to the even value"""
    x = np.array([1.0, -1.0, 1.5, -1.5, np.nan, 0.0, -0.0, 0.5/32768, 1.5/32768, -0.5/32768, -1.5/32768, 2.5/32768, 32766.5/32768, np.inf, -np.inf])
    want = [32767, -32768, 32767, -32768, 0, 0, 0, 0, 2, 0, -2, 2, 32766, 32767, -32768]
    for dtype in (np.float32, np.float64):
        got = mjpeg.pcm_s16(x.astype(dtype))
        assert got.dtype == np.dtype("<i2") and got.tolist() == want == A.s16(x.astype(dtype)).tolist()
    assert mjpeg.pcm_s16(np.zeros((5, 2), np.float32)).shape == (5, 2)
    track = mjpeg.SoundTrack(np.array([0.25, -0.25, np.nan], np.float32), 8000)      # one dimension: mono
    assert (track.channels, track.block, track.pcm.tolist()) == (1, 2, [[8192], [-8192], [0]])
    with pytest.raises(ValueError, match="sound track"):
        mjpeg.SoundTrack(np.zeros((4, 2, 2), np.float32), 8000)


def test_a_16_bit_wav_round_trips(tmp_path):
    """read_wav divides by 32768, pcm_s16 multiplies by it: every 16-bit value comes back as itself"""
    from shaderflow_amd.audio.reader import read_wav
    pcm = np.arange(-32768, 32768, dtype="<i2").reshape(-1, 2)
    data = pcm.tobytes()
    header = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(data), b"WAVE", b"fmt ", 16, 1, 2, 22050, 22050*4, 4, 16, b"data", len(data))
    (tmp_path/"all.wav").write_bytes(header + data)
    samples, samplerate = read_wav(tmp_path/"all.wav")
    assert samplerate == 22050 and samples.dtype == np.float32 and samples.shape == pcm.shape
    assert np.array_equal(mjpeg.pcm_s16(samples), pcm)


def test_the_limit_counts_the_audio(tmp_path):
    """Six frames of 100 bytes with 534 / 532 bytes of audio each, and a limit with room for frame 3 but not for the audio behind it: the
    file closes, valid, with three frames and their audio, and the RuntimeError says so"""
    fps, samplerate = 30, 8000
    samples = clip(2000, 1)
    track = mjpeg.SoundTrack(samples, samplerate)
    payloads = [bytes([k + 1])*100 for k in range(6)]
    audio = [2*(A.a(k + 1, samplerate, fps, 2000) - A.a(k, samplerate, fps, 2000)) for k in range(6)]
    assert audio == [532, 534, 534, 532, 534, 534]
    start = len(mjpeg.AviWriter(0, 16, 16, fps, track=track).headers(0, 0, 0, 0))
    three = sum(108 + 8 + n for n in audio[:3])
    limit = start - 8 + three + 108 + 8 + 16*7 + 200                   # frame 3 alone would fit with its index entry; its audio's 540 + 16 do not
    with pytest.raises(RuntimeError, match=r"closed at frame 3 of 6.*\.mjpeg"):
        write(tmp_path/"limit.avi", fps, track, payloads, limit=limit, width=16, height=16)
    data = (tmp_path/"limit.avi").read_bytes()
    avi = A.parse(data)
    assert len(data) - 8 == start - 8 + three + 8 + 16*6 <= limit
    assert len(data) - 8 + 108 + 8 + audio[3] + 32 > limit
    assert A.video(avi) == payloads[:3] and A.order(avi) == audio[:3]
    assert A.audio(avi) == A.s16(samples[:A.a(3, samplerate, fps, 2000)]).tobytes()
    A.check_streams(avi, 16, 16, fps, 3, 1, samplerate, A.a(3, samplerate, fps, 2000))
    # with room for exactly that audio and its index entry, frame 3 is in
    with pytest.raises(RuntimeError, match="closed at frame 4 of 6"):
        write(tmp_path/"four.avi", fps, track, payloads, limit=start - 8 + three + 108 + 8 + audio[3] + 8 + 16*8, width=16, height=16)
    assert A.order(A.parse((tmp_path/"four.avi").read_bytes())) == audio[:4]


@pytest.mark.parametrize("case", list(CASES))
def test_decode_audio_reads_the_track(case, tmp_path):
    from shaderflow_amd.audio.reader import decode_audio
    fps, samplerate, channels, total = CASES[case]
    samples = clip(total, channels)
    write(tmp_path/"clip.avi", fps, mjpeg.SoundTrack(samples, samplerate))
    got, rate = decode_audio(tmp_path/"clip.avi")
    end = A.a(7, samplerate, fps, total)
    assert rate == samplerate and got.dtype == np.float32 and got.shape == (end, channels)
    assert np.array_equal(got, A.s16(samples[:end]).astype(np.float32)/np.float32(32768))
    assert np.array_equal(mjpeg.pcm_s16(got), A.s16(samples[:end]))


def rec_avi(streams, movi: bytes) -> bytes:
    """A hand-made AVI: `streams` = [(fccType, strf bytes)], `movi` the list's content behind its fourcc"""
    def piece(fourcc, body):
        return fourcc + struct.pack("<I", len(body)) + body + b"\0"*(len(body) & 1)
    strls = b"".join(piece(b"LIST", b"strl" + piece(b"strh", struct.pack(A.STRH, kind, b"\0"*4, 0, 0, 0, 0, 1, 8000, 0, 0, 0, 0, 0, 0, 0, 0, 0)) + piece(b"strf", strf))
                     for kind, strf in streams)
    body = b"AVI " + piece(b"LIST", b"hdrl" + piece(b"avih", bytes(56)) + strls) + piece(b"LIST", b"movi" + movi)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_decode_audio_walks_rec_lists_and_the_pcm_formats(tmp_path):
    """The first `auds` stream is stream 1 here (`01wb`), its chunks lie in `movi` and in `rec ` lists, another stream's are skipped;
    8/24/32-bit integers and 32/64-bit floats convert as they do in a WAV file"""
    from shaderflow_amd.audio.reader import decode_audio, pcm_to_float

    def piece(fourcc, body):
        return fourcc + struct.pack("<I", len(body)) + body + b"\0"*(len(body) & 1)
    values = np.array([0.5, -0.25, 0.125, -1.0, 0.75, 0.0])
    encodings = {(1, 8): (values*128 + 128).astype(np.uint8).tobytes(), (1, 16): (values*32768).astype("<i2").tobytes(),
                 (1, 24): b"".join(struct.pack("<i", int(v*8388608))[:3] for v in values), (1, 32): (values*2147483648).astype("<i4").tobytes(),
                 (3, 32): values.astype("<f4").tobytes(), (3, 64): values.astype("<f8").tobytes()}
    for (tag, bits), raw in encodings.items():
        block = bits//8*2
        strf = struct.pack("<HHIIHH", tag, 2, 8000, 8000*block, block, bits)
        third = len(raw)//3
        movi = (piece(b"00dc", b"\xff\xd8") + piece(b"01wb", raw[:third]) + piece(b"02wb", b"\x55"*6) +
                piece(b"LIST", b"rec " + piece(b"00dc", b"\xff\xd8\xff") + piece(b"01wb", raw[third:2*third])) + piece(b"01wb", raw[2*third:]))
        path = tmp_path/f"{tag}-{bits}.avi"
        path.write_bytes(rec_avi([(b"vids", bytes(40)), (b"auds", strf), (b"auds", strf)], movi))
        got, rate = decode_audio(path)
        assert rate == 8000 and got.shape == (3, 2), (tag, bits)
        assert np.array_equal(got.ravel(), values.astype(np.float32)), (tag, bits)
        assert np.array_equal(got.ravel(), pcm_to_float(raw, tag, bits, path))


def test_an_avi_without_pcm_audio_goes_to_the_ffmpeg_branch(tmp_path, monkeypatch):
    """No `auds` stream (the silent export), or a compressed one: as any unknown container, which without ffmpeg is the ValueError"""
    import shutil

    from shaderflow_amd.audio.reader import decode_audio
    monkeypatch.setattr(shutil, "which", lambda name: None)
    write(tmp_path/"silent.avi", 30, None)
    (tmp_path/"mp3.avi").write_bytes(rec_avi([(b"vids", bytes(40)), (b"auds", struct.pack("<HHIIHH", 0x55, 2, 44100, 16000, 1, 0))], b"" + b"01wb" + struct.pack("<I", 4) + b"abcd"))
    for name in ("silent.avi", "mp3.avi"):
        with pytest.raises(ValueError, match="no ffmpeg/ffprobe binary"):
            decode_audio(tmp_path/name)


def test_the_avi_reader_skips_the_audio(tmp_path):
    """mjpegsource.AviReader on the two-stream file: the same frames, sizes and fps as on the silent one"""
    from shaderflow_amd.mjpegsource import AviReader
    from tests import jpeg_ref as J
    fps = Fraction(2997, 100)
    pictures = [J.encode(J.picture(kind, 16, 16, seed=k), quality) for k, (kind, quality) in enumerate((("gradient", 90), ("noise", 25), ("checker", 50)))]
    assert len({len(p) & 1 for p in pictures}) == 2, "odd and even"
    silent = write(tmp_path/"silent.avi", fps, None, pictures, width=16, height=16)
    sound = write(tmp_path/"sound.avi", fps, mjpeg.SoundTrack(clip(3000, 1), 8000), pictures, width=16, height=16)
    one, two = AviReader(tmp_path/"silent.avi"), AviReader(tmp_path/"sound.avi")
    assert two.fps == one.fps == pytest.approx(29.97) and len(two.index) == len(one.index) == 3
    assert [size for _, size in two.index] == [size for _, size in one.index] == [len(p) for p in pictures]
    assert [sound[at:at + size] for at, size in two.index] == [silent[at:at + size] for at, size in one.index] == pictures
    assert (two.width, two.height) == (one.width, one.height) == (16, 16)
    first = A.parse(sound)["start"]
    assert [at for at, _ in two.index] == [first + offset + 4 for fourcc, offset, _ in A.parse(sound)["chunks"] if fourcc == b"00dc"]


PARENT_HEADERS = bytes.fromhex(
    "5249464642020000415649204c495354c00000006864726c6176696838000000578200000000000000000000100000000600000000000000010000006400000060000000"
    "40000000000000000000000000000000000000004c495354740000007374726c7374726838000000766964734d4a504700000000000000000000000064000000b50b0000"
    "000000000600000064000000ffffffff0000000000000000600040007374726628000000280000006000000040000000010018004d4a5047004800000000000000000000"
    "00000000000000004c495354060100006d6f7669")


def test_without_a_track_the_bytes_are_the_old_ones(tmp_path):
    """96 x 64 at 29.97 fps, payloads of 1, 2, 7, 100, 33 and 64 bytes: the headers are the ones the class wrote before it knew of sound
    tracks (recorded from it), and behind them stand the `00dc` chunks and their idx1 alone"""
    payloads = PAYLOADS[:6]
    data = write(tmp_path/"silent.avi", 29.97, None, payloads)
    movi = b"".join(b"00dc" + struct.pack("<I", len(p)) + p + b"\0"*(len(p) & 1) for p in payloads)
    index, offset = b"", 4
    for p in payloads:
        index += struct.pack("<4sIII", b"00dc", 0x10, offset, len(p))
        offset += 8 + len(p) + (len(p) & 1)
    assert len(PARENT_HEADERS) == 224 and data == PARENT_HEADERS + movi + b"idx1" + struct.pack("<I", len(index)) + index
    assert data == write(tmp_path/"none.avi", 29.97, None, payloads, mode="sizes") and len(data) == 586


def test_the_refusals_need_no_device(tmp_path):
    """sound_track with a sink that cannot hold it is refused where suffix and pixel format are judged, before anything touches the GPU;
    the message names the `.avi` requirement and, for the ffmpeg branch, the hook that already attaches the file"""
    from types import SimpleNamespace

    from shaderflow_amd.exporting import ExportingHelper
    scene = SimpleNamespace(width=40, height=24, fps=30.0, runtime=1.0, modules=[], ffmpeg=SimpleNamespace(time=0))
    for output in ("pipe", tmp_path/"clip.mjpeg", tmp_path/"clip.mjpg"):
        with pytest.raises(ValueError, match=r"sound_track.*\.avi"):
            ExportingHelper(scene, pixel_format="mjpeg", sound_track=True).ffmpeg_output(output)
    for pixel_format in ("yuv420p", "rgb24"):
        with pytest.raises(ValueError, match=r"sound_track.*\.avi.*ffhook"):
            ExportingHelper(scene, pixel_format=pixel_format, sound_track=True).ffmpeg_output(tmp_path/"clip.avi")
    with pytest.raises(ValueError, match="no audio module"):
        ExportingHelper(scene, pixel_format="mjpeg", sound_track=True).ffmpeg_output(tmp_path/"clip.avi")
    with pytest.raises(ValueError, match="no audio module 'iAudio'"):
        ExportingHelper(scene, pixel_format="mjpeg", sound_track="iAudio").ffmpeg_output(tmp_path/"clip.avi")
    helper = ExportingHelper(scene, pixel_format="mjpeg")
    helper.ffmpeg_output(tmp_path/"clip.avi")
    assert not helper.wants_track and helper._track is None
