"""
OpenDML (AVI 2.0) without a GPU: `mjpeg.segment_cuts` (the rule), `AviWriter(..., opendml=budget)` through `add()` and through
`finish(sizes)` on a sparse file past 4 GiB, the layout function at size without a file, the readers (`clips.AviClip` under
`mjpegsource.AviReader` and `pngsource.AviReader`, `decode_audio`) over `RIFF 'AVIX'` segments, and the native rule of
csrc/ring_segments.hpp as a program of its own. tests/odml_ref.py is the independent parser; tests/avi_ref.py reads the AVI 1.0 twin.
"""
import os
import random
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from shaderflow_amd import mjpeg
from tests import avi_ref as A
from tests import jpeg_ref as J
from tests import odml_ref as O
from tests import png_ref as P

ROOT = Path(__file__).resolve().parent.parent
FPS, RATE = 30.0, 8000


def rule(runs, start, budget):
    """The issue's rule, restated: (cuts, where every frame's run begins, the end)"""
    pos, seg_start, in_seg, cuts, places = start, 0, 0, [], []
    for j, run in enumerate(runs):
        if in_seg > 0 and pos + run - seg_start > budget:
            seg_start, pos, in_seg = pos, pos + 24, 0
            cuts.append(j)
        places.append(pos)
        pos, in_seg = pos + run, in_seg + 1
    return cuts, places, pos


def payloads(count=24, low=4100, high=6000, seed=5):
    rng = np.random.default_rng(seed)
    found = [rng.integers(0, 256, int(size), dtype=np.uint8).tobytes() for size in rng.integers(low, high, count)]
    found[1], found[2] = found[1][:low + 1], found[2][:low + 2]         # sizes of both parities
    return found


def track_of(kind):
    if kind is None:
        return None
    frames = {"full": 8000, "short": 2000}[kind]                       # 24 frames at 30 fps are 6 400 sample frames; the short one ends in frame 7
    rng = np.random.default_rng(11)
    return mjpeg.SoundTrack(rng.uniform(-1, 1, (frames, 2)), RATE)


def shares(kind, count):
    total = {None: 0, "full": 8000, "short": 2000}[kind]
    return [4*(A.a(k + 1, RATE, FPS, total) - A.a(k, RATE, FPS, total)) for k in range(count)]


def runs_of(sizes, sound):
    return [8 + size + (size & 1) + ((8 + share + (share & 1)) if share else 0) for size, share in zip(sizes, sound)]


def write(path, frames, track=None, opendml=None, fourcc=b"MJPG", width=48, height=32):
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        writer = mjpeg.AviWriter(fd, width, height, FPS, track=track, fourcc=fourcc, opendml=opendml)
        writer.begin()
        for frame in frames:
            writer.add(frame)
        try:
            writer.finish()
        finally:
            assert os.lseek(fd, 0, os.SEEK_CUR) == os.fstat(fd).st_size  # the descriptor is left at the file's end
    finally:
        os.close(fd)
    return writer


# ---- the rule ------------------------------------------------------------------------------------------------------------------------

def test_the_rule_on_hand_made_runs():
    cuts = mjpeg.segment_cuts
    assert cuts([], 100, 4096) == [] and cuts([10], 100, 4096) == []
    assert cuts([100, 200, 300], 400, 1000) == []                      # an exact fit: 400 + 600 = 1000
    assert cuts([100, 200, 301], 400, 1000) == [2]                     # one byte more
    assert cuts([100, 200, 300, 676, 1], 400, 1000) == [3]
    assert cuts([100, 200, 300, 976, 1], 400, 1000) == [3, 4] and cuts([100, 200, 300, 975, 1], 400, 1000) == [3]   # the gap's 24 bytes count
    assert cuts([10, 5000, 10, 10], 400, 1000) == [1, 2]               # a run larger than the budget sits alone
    assert cuts([5000, 10], 400, 1000) == [1] and cuts([5000], 400, 1000) == []
    assert cuts([10, 10, 10], 4000, 1000) == [1]                       # a budget smaller than `start`: frame 0 is in segment 0 all the same
    for runs, start, budget in [([100, 200, 300, 676, 1], 400, 1000), ([7]*50, 0, 64), ([10, 5000, 10, 10], 400, 1000)]:
        assert cuts(runs, start, budget) == rule(runs, start, budget)[0]
    assert cuts(iter([100, 200, 301]), 400, 1000) == [2]               # any iterable
    assert mjpeg.SEGMENT_BYTES == 1 << 30 and mjpeg.SUPER_ENTRIES == 256


@pytest.mark.parametrize("value", [0, 100, 4095, (1 << 31) + 1, 1.5, "1G"])
def test_a_segment_size_out_of_range_is_refused(value, tmp_path):
    with pytest.raises(ValueError, match="opendml"):
        mjpeg.AviWriter(None, 48, 32, FPS, opendml=value)
    assert mjpeg.check_opendml(True) == 1 << 30 and mjpeg.check_opendml(False) is None and mjpeg.check_opendml(None) is None
    assert mjpeg.check_opendml(4096) == 4096 and mjpeg.check_opendml(1 << 31) == 1 << 31


# ---- the writer through add() --------------------------------------------------------------------------------------------------------

_twins: dict = {}


def twin(kind, tmp_path_factory):
    """The AVI 1.0 file of the 24 payloads with this track, and the same as OpenDML in one segment: made once per track"""
    if kind not in _twins:
        folder = tmp_path_factory.mktemp(f"twin-{kind}")
        frames = payloads()
        write(folder/"one.avi", frames, track_of(kind))
        write(folder/"whole.avi", frames, track_of(kind), opendml=1 << 31)
        _twins[kind] = (A.parse((folder/"one.avi").read_bytes()), (folder/"whole.avi").read_bytes())
    return _twins[kind]


@pytest.mark.parametrize("budget_kind", ["two-fit", "two-less-one", "frame-each", "whole"])
@pytest.mark.parametrize("kind", [None, "full", "short"], ids=["silent", "track", "short-track"])
def test_the_writer_through_add(kind, budget_kind, tmp_path, tmp_path_factory):
    frames = payloads()
    sizes, sound = [len(frame) for frame in frames], shares(kind, len(frames))
    runs = runs_of(sizes, sound)
    old, whole = twin(kind, tmp_path_factory)
    start = O.parse(whole)["movis"][0] + 4
    budget = {"two-fit": start + runs[0] + runs[1], "two-less-one": start + runs[0] + runs[1] - 1, "frame-each": min(runs) - 1,
              "whole": len(whole) + 1}[budget_kind]
    writer = write(tmp_path/"clip.avi", frames, track_of(kind), opendml=budget)
    assert writer.start == start
    data = (tmp_path/"clip.avi").read_bytes()
    avi = O.parse(data)                                                # the walk and the indexes agree, every size closes, every count holds
    cuts, places, end = rule(runs, start, budget)
    assert cuts == mjpeg.segment_cuts(runs, start, budget)
    assert cuts[:1] == {"two-fit": [2], "two-less-one": [1], "frame-each": [1], "whole": []}[budget_kind]
    assert budget_kind != "frame-each" or cuts == list(range(1, 24))
    bounds = [0, *cuts, len(frames)]
    assert [len(mine) for mine in avi["per_segment"][b"00dc"]] == [b - a for a, b in zip(bounds[:-1], bounds[1:])]
    assert [at for at, _ in avi["walk"][b"00dc"]] == [place + 8 for place in places]
    assert [begin for begin, _, _ in avi["riffs"]][1:] == [places[j] - 24 for j in cuts]
    # the payloads and the audio are the AVI 1.0 writer's on the same input
    assert O.payloads(data, avi["walk"][b"00dc"]) == A.video(old) == frames
    if kind is None:
        assert list(avi["walk"]) == [b"00dc"] and avi["avih"][3] == 0x10 and avi["avih"][6] == 1
    else:
        assert b"".join(O.payloads(data, avi["walk"][b"01wb"])) == A.audio(old) == track_of(kind).pcm[:sum(sound)//4].tobytes()
        assert [size for _, size in avi["walk"][b"01wb"]] == [share for share in sound if share]
        assert avi["avih"][3] == 0x110 and avi["avih"][6] == 2
        assert avi["streams"][1]["strh"]["length"] == sum(sound)//4 == old["streams"][1]["strh"]["length"]
        assert avi["streams"][1]["strf"] == old["streams"][1]["strf"]
        assert avi["streams"][1]["strh"]["suggested_buffer"] == max(sound)
    # the counts as defined, and the stream header otherwise the AVI 1.0 file's
    assert avi["total"] == avi["streams"][0]["strh"]["length"] == 24 and avi["avih"][4] == bounds[1]
    assert avi["streams"][0]["strh"] == old["streams"][0]["strh"] and avi["streams"][0]["strf"] == old["streams"][0]["strf"]
    assert avi["avih"][:4] + avi["avih"][5:] == old["avih"][:4] + old["avih"][5:]
    # every RIFF chunk but the last spans at most the budget, unless one frame alone is larger; the last passes it by its index chunks
    held = [b - a for a, b in zip(bounds[:-1], bounds[1:])]
    assert all(span <= budget or count == 1 for span, count in zip(O.spans(avi)[:-1], held[:-1]))
    tail = sum(size for _, _, size, _, _ in avi["standard"])
    assert tail == sum(32 for _ in avi["standard"]) + 8*(24 + sum(1 for share in sound if share))
    assert O.spans(avi)[-1] - tail <= budget or held[-1] == 1
    if budget_kind == "whole":
        assert len(avi["riffs"]) == 1 and b"AVIX" not in data and [len(s["super"]) for s in avi["streams"]] == [1]*len(avi["streams"])
        assert data == whole                                           # (the budget is in no byte of the file)
    if kind == "short" and budget_kind != "whole":
        # the track ends in frame 7: later segments have no ix01 and no super-index entry
        with_audio = sum(1 for a, b in zip(bounds[:-1], bounds[1:]) if any(sound[a:b]))
        assert len(avi["streams"][1]["super"]) == with_audio < len(avi["riffs"]) == len(avi["streams"][0]["super"])
        assert [name for name, *_ in avi["standard"]].count(b"ix01") == with_audio


def test_without_the_argument_the_file_is_the_one_it_was(tmp_path):
    frames = payloads(6)
    write(tmp_path/"default.avi", frames, track_of("full"))
    write(tmp_path/"none.avi", frames, track_of("full"), opendml=None)
    data = (tmp_path/"default.avi").read_bytes()
    assert data == (tmp_path/"none.avi").read_bytes() and not any(word in data for word in (b"indx", b"odml", b"AVIX", b"ix00"))
    A.parse(data)


def test_the_cap(tmp_path):
    """300 frames, one per segment: the file is closed, valid, with the 256 frames of segments 0 to 255, and the error names frame 256"""
    frames = payloads(300, 4100, 4200, seed=2)
    with pytest.raises(RuntimeError, match=r"closed at frame 256 of 300; a larger segment size .* holds the whole export"):
        write(tmp_path/"clip.avi", frames, opendml=4096)
    data = (tmp_path/"clip.avi").read_bytes()
    avi = O.parse(data)
    assert len(avi["riffs"]) == 256 == len(avi["streams"][0]["super"]) and avi["total"] == 256 and avi["avih"][4] == 1
    assert O.payloads(data, avi["walk"][b"00dc"]) == frames[:256]


# ---- the layout at size --------------------------------------------------------------------------------------------------------------

def test_the_layout_of_ten_thousand_frames_without_a_file():
    """10 000 frames of 600 000 bytes at the default budget: six segments; the index chunks and the last segment lie past 2^32, in
    qwOffset and qwBaseOffset, and every dwOffset is a 32-bit number"""
    writer = mjpeg.AviWriter(None, 3840, 2160, 60.0, opendml=True)
    plan = writer.layout([600000]*10000)
    start = len(writer.headers(0, 0, 0, 0))
    cuts, places, end = rule([600008]*10000, start, 1 << 30)
    assert plan.cuts == cuts and len(plan.spans) == 6 and plan.fit == 10000 and plan.data_end == end > 1 << 32
    assert [begin for begin, _ in plan.spans] == [0] + [places[j] - 24 for j in cuts]
    assert all(b - a <= 1 << 30 for a, b in plan.spans[:-1]) and plan.spans[-1][1] == end + len(plan.tail)
    assert len(plan.supers[0]) == 6 and plan.supers[1] == [] and sum(duration for _, _, duration in plan.supers[0]) == 10000
    assert all(offset > 1 << 32 for offset, _, _ in plan.supers[0])   # qwOffset: the ix00 chunks stand behind 6 GB of frames
    at, bases = 0, []
    for number, (offset, size, duration) in enumerate(plan.supers[0]):
        assert offset == end + at and plan.tail[at:at + 4] == b"ix00" and struct.unpack("<I", plan.tail[at + 4:at + 8])[0] == size - 8
        longs, subtype, kind, used, name, base, reserved = struct.unpack("<HBBI4sQI", plan.tail[at + 8:at + 32])
        assert (longs, subtype, kind, used, name, reserved) == (2, 0, 1, duration, b"00dc", 0) and base == plan.movis[number]
        entries = np.frombuffer(plan.tail, "<u4", 2*used, at + 32).reshape(used, 2)
        first = 0 if number == 0 else cuts[number - 1]
        assert [int(base) + int(o) for o in entries[:, 0]] == [place + 8 for place in places[first:first + used]]
        assert int(entries[:, 0].max()) < 1 << 30 and set(entries[:, 1].tolist()) == {600000}
        bases.append(base)
        at += size
    assert at == len(plan.tail) and bases[-1] > 1 << 32 and bases == sorted(bases)
    head = writer.opendml_headers(plan)
    assert len(head) == start and struct.unpack("<I", head[4:8])[0] == plan.spans[0][1] - 8
    assert head.count(b"indx") == 1 and struct.unpack("<Q", head[head.index(b"indx") + 32:head.index(b"indx") + 40])[0] == plan.supers[0][0][0]


# ---- a file past 4 GiB, sparse -------------------------------------------------------------------------------------------------------

def test_a_sparse_file_past_four_gib(tmp_path):
    """begin(), then only the chunk headers and a few payload bytes at their places — frame 0 a real JPEG, six frames of about 900 MB
    that stay holes (six of 700 MB end below 2^32; 900 MB still leaves two to a segment impossible and puts the last frame's first byte
    past 2^32) — then finish(sizes): odml_ref and AviClip agree on where the frames are, the later offsets exceed 2^32 and the bytes
    there are the ones written. The clip is not iterated."""
    from shaderflow_amd import mjpegsource as M
    first = J.encode(J.picture("gradient", 48, 32), 50)
    sizes = [len(first)] + [900_000_001 + 1000*k for k in range(6)]
    fd = os.open(tmp_path/"large.avi", os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        writer = mjpeg.AviWriter(fd, 48, 32, FPS, opendml=True)
        writer.begin()
        cuts, places, end = rule(runs_of(sizes, [0]*7), writer.start, 1 << 30)
        assert cuts == [2, 3, 4, 5, 6] and end > 1 << 32
        marks = [b"frame %d begins" % k for k in range(7)]
        try:
            os.pwrite(fd, b"00dc" + struct.pack("<I", sizes[0]) + first, places[0])
            for k in range(1, 7):
                os.pwrite(fd, b"00dc" + struct.pack("<I", sizes[k]) + marks[k], places[k])
                os.pwrite(fd, b"ends", places[k] + 8 + sizes[k] - 4)
            writer.finish(sizes)
        except OSError as error:
            pytest.skip(f"the temporary file system refuses a sparse file of {end} bytes: {error}")
    finally:
        os.close(fd)
    import mmap
    with open(tmp_path/"large.avi", "rb") as file, mmap.mmap(file.fileno(), 0, access=mmap.ACCESS_READ) as data:
        assert len(data) > 1 << 32
        avi = O.parse(data)
        found = avi["walk"][b"00dc"]
        assert found == [(place + 8, size) for place, size in zip(places, sizes)] and len(avi["riffs"]) == 6
        assert [begin for begin, _, _ in avi["riffs"]][1:] == [places[j] - 24 for j in cuts]
        assert found[-1][0] > 1 << 32 and avi["streams"][0]["super"][-1][0] > 1 << 32
        for k in range(1, 7):
            at, size = found[k]
            assert bytes(data[at:at + len(marks[k])]) == marks[k] and bytes(data[at + size - 4:at + size]) == b"ends"
        assert avi["total"] == 7 and avi["avih"][4] == 2
    reader = M.AviReader(tmp_path/"large.avi")
    try:
        assert reader.index == found and len(reader) == 7 and (reader.width, reader.height) == (48, 32) and reader.largest == sizes[-1]
    finally:
        reader.close()


# ---- reading -------------------------------------------------------------------------------------------------------------------------

def test_a_written_file_reads_back_frame_for_frame(tmp_path):
    from shaderflow_amd import mjpegsource as M
    from shaderflow_amd import pngsource
    from shaderflow_amd.audio.reader import decode_audio
    track = track_of("full")
    jpegs = [J.encode(J.picture("noise", 48, 32, seed), 90) for seed in range(9)]
    pngs = [P.encode(P.picture("noise", 48, 32, seed)) for seed in range(9)]
    for name, frames, fourcc, reader_of in (("jpeg.avi", jpegs, b"MJPG", M.AviReader), ("png.avi", pngs, b"MPNG", pngsource.AviReader)):
        write(tmp_path/name, frames, track, opendml=3*max(map(len, frames)), fourcc=fourcc)
        data = (tmp_path/name).read_bytes()
        assert len(O.parse(data)["riffs"]) >= 3
        reader = reader_of(tmp_path/name)
        assert len(reader) == 9 and reader.largest == max(map(len, frames)) and abs(reader.fps - FPS) < 1e-9
        assert list(reader) == frames
        got, rate = decode_audio(tmp_path/name)
        share = A.a(9, RATE, FPS, 8000)
        assert rate == RATE and np.array_equal(got, track.pcm[:share].astype(np.float32)/np.float32(32768))
        # a last segment cut mid-chunk: the frames that are whole
        last = O.parse(data)["walk"][b"00dc"][-1]
        (tmp_path/("cut-" + name)).write_bytes(data[:last[0] + last[1]//2])
        assert list(reader_of(tmp_path/("cut-" + name))) == frames[:8]
        # an AVIX chunk without a movi list is skipped, and says so; the segments behind it are still read
        stub = b"RIFF" + struct.pack("<I", 12) + b"AVIX" + b"JUNK" + struct.pack("<I", 0)
        second = O.parse(data)["riffs"][1][0]
        (tmp_path/("stub-" + name)).write_bytes(data[:second] + stub + data[second:])
        with pytest.warns(UserWarning, match="AVIX"):
            assert list(reader_of(tmp_path/("stub-" + name))) == frames


def test_rec_lists_and_junk_in_a_segment_are_walked_and_skipped(tmp_path):
    """What other writers put into `AVIX` chunks: `rec ` lists around the chunks, JUNK between them, an audio stream's chunks"""
    from shaderflow_amd import mjpegsource as M
    jpegs = [J.encode(J.picture("noise", 48, 32, seed), 90) for seed in range(4)]
    write(tmp_path/"one.avi", jpegs[:2])
    body = b"JUNK" + struct.pack("<I", 3) + b"abc\0" + mjpeg.chunk(jpegs[2]) + b"01wb" + struct.pack("<I", 2) + b"zz"
    rec = b"rec " + mjpeg.chunk(jpegs[3]) + b"ix00" + struct.pack("<I", 4) + b"\0\0\0\0"
    movi = b"movi" + body + b"LIST" + struct.pack("<I", len(rec)) + rec
    avix = b"AVIX" + b"JUNK" + struct.pack("<I", 4) + b"0000" + b"LIST" + struct.pack("<I", len(movi)) + movi
    (tmp_path/"more.avi").write_bytes((tmp_path/"one.avi").read_bytes() + b"RIFF" + struct.pack("<I", len(avix)) + avix)
    assert list(M.AviReader(tmp_path/"more.avi")) == jpegs


# ---- the native rule, alone ----------------------------------------------------------------------------------------------------------

def test_the_native_rule_agrees_with_segment_cuts(tmp_path):
    """tests/ring_segments_check.cpp and csrc/ring_segments.hpp alone, under the address and undefined-behaviour sanitizers, as a process
    of its own: the hand-made cases above, positions past 2^32, and 300 seeded random ones"""
    compiler = shutil.which("g++")
    if compiler is None:
        pytest.skip("no g++")
    program = tmp_path/"ring_segments_check"
    built = subprocess.run([compiler, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan",     # the runtimes in the program itself: it needs nothing from its environment
                            "-I", str(ROOT/"shaderflow_amd"/"csrc"), str(ROOT/"tests"/"ring_segments_check.cpp"), "-o", str(program)],
                           capture_output=True, text=True)
    if built.returncode and any(word in built.stderr for word in ("-lasan", "-lubsan", "libasan", "libubsan")):
        pytest.skip("g++ lacks the sanitizer runtime")
    assert built.returncode == 0, built.stderr
    cases = [([100, 200, 300], 400, 1000), ([100, 200, 301], 400, 1000), ([100, 200, 300, 676, 1], 400, 1000), ([10, 5000, 10, 10], 400, 1000),
             ([5000, 10], 400, 1000), ([10, 10, 10], 4000, 1000), ([], 0, 4096), ([600008]*10000, 4620, 1 << 30),
             ([750_000_010]*7, 4620, 1 << 30), ([(1 << 32) - 2, (1 << 32) - 2, 10], 4620, 1 << 31)]
    rng = random.Random(20)
    for _ in range(300):
        budget = rng.choice([4096, 5000, 65536, 1 << 20])
        runs = [rng.choice([rng.randrange(8, 64), rng.randrange(8, budget//3), rng.randrange(8, 2*budget)]) & ~1 for _ in range(rng.randrange(0, 60))]
        cases.append((runs, rng.choice([0, 212, 4620, budget - 8, budget, 3*budget]), budget))
    text = "".join(f"{start} {budget} 24 {len(runs)} {' '.join(map(str, runs))}\n" for runs, start, budget in cases)
    ran = subprocess.run([str(program)], input=text, capture_output=True, text=True)
    assert ran.returncode == 0, ran.stderr
    lines = ran.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, (runs, start, budget) in zip(lines, cases):
        words = line.split()
        assert words[0] == "cuts" and words[-2] == "end"
        want = mjpeg.segment_cuts(runs, start, budget)
        assert [int(word) for word in words[1:-2]] == want
        assert int(words[-1]) == start + sum(runs) + 24*len(want)
