"""
An OpenDML (AVI 2.0) file taken apart, written against the OpenDML 1.02 text and not against shaderflow_amd/mjpeg.py: further
`RIFF 'AVIX'` chunks behind the `RIFF 'AVI '` chunk, each with a `movi` list, and per stream a two-level 64-bit index — `indx` (an index
of indexes) in the stream's header list, and the `ix##` standard index chunks it points to.

`parse(data)` takes `bytes` or a memory map (a file past 4 GiB, sparse: only chunk headers are read, never a payload) and returns the
chunks of every stream twice — found by walking every `movi`, and found by following `indx` → `ix##` → entries — with the structure
checked on the way: every RIFF and LIST size closes exactly on the next chunk or the file's end, the `indx` headers, counts and
durations, base offsets that point at `movi` fourccs, `dwSize` of a super-index entry = the index chunk's size + 8.
"""
import struct

STRH = "<4s4sIHHIIIIIIII4H"
STRH_FIELDS = ("type", "handler", "flags", "priority", "language", "initial_frames", "scale", "rate", "start", "length",
               "suggested_buffer", "quality", "sample_size", "left", "top", "right", "bottom")
SUPER_ENTRIES = 256


def u32(data, at: int) -> int:
    return struct.unpack("<I", data[at:at + 4])[0]


def children(data, first: int, last: int) -> list:
    """[(fourcc, body offset, size)] of the chunks that fill [first, last) exactly; the pad byte of an odd chunk is zero"""
    found, pos = [], first
    while pos < last:
        assert pos + 8 <= last, (pos, last)
        fourcc, size = bytes(data[pos:pos + 4]), u32(data, pos + 4)
        assert pos + 8 + size + (size & 1) <= last, (fourcc, size, pos, last)
        if size & 1:
            assert data[pos + 8 + size] == 0, "the pad byte is zero"
        found.append((fourcc, pos + 8, size))
        pos += 8 + size + (size & 1)
    assert pos == last, (pos, last)
    return found


def parse(data) -> dict:
    """{"avih": 14 ints, "streams": [{"strh": {...}, "strf": bytes, "super": [(qwOffset, dwSize, dwDuration)], "id": b"00dc"}],
    "total": dmlh's dwTotalFrames, "riffs": [(offset, end, form)], "movis": [offset of the fourcc], "walk": {id: [(data offset, size)]},
    "indexed": {id: [(data offset, size)]}, "per_segment": {id: [chunks of that stream in segment k]}, "standard": [(fourcc, offset,
    size with header, segment, entries)]}"""
    out = {"streams": [], "riffs": [], "movis": [], "walk": {}, "indexed": {}, "per_segment": {}, "standard": []}
    # the top level: RIFF chunks that close on one another and on the file's end
    pos = 0
    while pos < len(data):
        assert bytes(data[pos:pos + 4]) == b"RIFF", pos
        end = pos + 8 + u32(data, pos + 4)
        assert end <= len(data) and end % 2 == 0, (pos, end, len(data))
        out["riffs"].append((pos, end, bytes(data[pos + 8:pos + 12])))
        pos = end
    assert pos == len(data)
    assert [form for _, _, form in out["riffs"]] == [b"AVI "] + [b"AVIX"]*(len(out["riffs"]) - 1)

    movi_spans = []
    for number, (begin, end, _) in enumerate(out["riffs"]):
        top = children(data, begin + 12, end)
        kinds = [bytes(data[body:body + 4]) if fourcc == b"LIST" else fourcc for fourcc, body, _ in top]
        assert kinds == ([b"hdrl", b"movi"] if number == 0 else [b"movi"]), kinds     # (no idx1: indx is the index)
        if number == 0:
            _, body, size = top[0]
            inner = children(data, body + 4, body + size)
            assert [name for name, _, _ in inner] == [b"avih"] + [b"LIST"]*(len(inner) - 1)
            out["avih"] = struct.unpack("<14I", data[inner[0][1]:inner[0][1] + inner[0][2]])
            lists = [(bytes(data[at:at + 4]), at, n) for _, at, n in inner[1:]]
            assert [kind for kind, _, _ in lists] == [b"strl"]*(len(lists) - 1) + [b"odml"]
            for stream, (_, at, n) in enumerate(lists[:-1]):
                leaves = children(data, at + 4, at + n)
                assert [name for name, _, _ in leaves] == [b"strh", b"strf", b"indx"]
                (_, h_at, h_n), (_, f_at, f_n), (_, x_at, x_n) = leaves
                assert h_n == struct.calcsize(STRH) and x_n == 24 + 16*SUPER_ENTRIES
                longs, subtype, kind, used, chunk_id, reserved = struct.unpack("<HBBI4s12s", data[x_at:x_at + 24])
                assert (longs, subtype, kind, reserved) == (4, 0, 0, b"\0"*12) and used <= SUPER_ENTRIES
                entries = [struct.unpack("<QII", data[x_at + 24 + 16*k:x_at + 40 + 16*k]) for k in range(SUPER_ENTRIES)]
                assert entries[used:] == [(0, 0, 0)]*(SUPER_ENTRIES - used), "unused entries are zero"
                strh = dict(zip(STRH_FIELDS, struct.unpack(STRH, data[h_at:h_at + h_n])))
                assert chunk_id == b"%02d" % stream + {b"vids": b"dc", b"auds": b"wb"}[strh["type"]]
                out["streams"].append({"strh": strh, "strf": bytes(data[f_at:f_at + f_n]), "super": entries[:used], "id": chunk_id})
            _, at, n = lists[-1]
            (name, d_at, d_n), = children(data, at + 4, at + n)
            assert name == b"dmlh" and d_n == 248 and bytes(data[d_at + 4:d_at + 248]) == b"\0"*244
            out["total"] = u32(data, d_at)
        _, body, size = top[-1]
        out["movis"].append(body)
        movi_spans.append((body + 4, body + size))
        assert body + size == end, "the movi list closes its RIFF chunk"
    assert len(out["streams"]) == out["avih"][6]

    # the walk: data chunks segment by segment; standard index chunks behind the last data chunk of the last segment only
    ids = [stream["id"] for stream in out["streams"]]
    out["walk"] = {name: [] for name in ids}
    out["per_segment"] = {name: [] for name in ids}
    for number, (first, last) in enumerate(movi_spans):
        found = children(data, first, last)
        names = [fourcc for fourcc, _, _ in found]
        data_chunks = [entry for entry in found if entry[0] in ids]
        assert data_chunks, "a segment holds at least one frame"
        tail = found[len(data_chunks):]
        assert names[:len(data_chunks)] == [entry[0] for entry in data_chunks], "index chunks stand behind the data chunks"
        assert all(fourcc[:2] == b"ix" for fourcc, _, _ in tail) and (not tail or number == len(movi_spans) - 1), names[len(data_chunks):]
        for name in ids:
            mine = [(at, size) for fourcc, at, size in data_chunks if fourcc == name]
            out["walk"][name] += mine
            out["per_segment"][name].append(mine)

    # the indexes: indx → ix## → entries
    for stream, record in enumerate(out["streams"]):
        name, block = record["id"], 1
        if record["strh"]["type"] == b"auds":
            block = struct.unpack("<HHIIHH", record["strf"][:16])[4]
        indexed, segments_seen = [], []
        for offset, size, duration in record["super"]:
            assert bytes(data[offset:offset + 4]) == b"ix%02d" % stream, (offset, bytes(data[offset:offset + 4]))
            assert size == u32(data, offset + 4) + 8, "dwSize counts the index chunk's header"
            assert movi_spans[-1][0] <= offset and offset + size <= movi_spans[-1][1], "the index chunks lie in the last movi"
            longs, subtype, kind, used, chunk_id, base, reserved = struct.unpack("<HBBI4sQI", data[offset + 8:offset + 32])
            assert (longs, subtype, kind, chunk_id, reserved) == (2, 0, 1, name, 0) and size == 32 + 8*used and used > 0
            assert base in out["movis"] and bytes(data[base:base + 4]) == b"movi", "qwBaseOffset is the file offset of a movi fourcc"
            segment = out["movis"].index(base)
            segments_seen.append(segment)
            entries = [struct.unpack("<II", data[offset + 32 + 8*k:offset + 40 + 8*k]) for k in range(used)]
            assert all(at < 1 << 32 and not length >> 31 for at, length in entries), "dwOffset is 32-bit, bit 31 of dwSize is clear"
            for at, length in entries:
                assert bytes(data[base + at - 8:base + at - 4]) == name and u32(data, base + at - 4) == length, (base, at, length)
            assert duration == (used if record["strh"]["type"] == b"vids" else sum(length for _, length in entries)//block)
            assert [(base + at, length) for at, length in entries] == out["per_segment"][name][segment], "an index chunk lists its segment's chunks"
            indexed += [(base + at, length) for at, length in entries]
            out["standard"].append((b"ix%02d" % stream, offset, size, segment, used))
        assert segments_seen == [k for k, mine in enumerate(out["per_segment"][name]) if mine], "one index chunk per segment that has chunks"
        out["indexed"][name] = indexed
        assert record["strh"]["length"] == sum(duration for _, _, duration in record["super"])
    assert out["indexed"] == out["walk"]
    video = [stream for stream in out["streams"] if stream["strh"]["type"] == b"vids"]
    assert out["total"] == video[0]["strh"]["length"] == len(out["walk"][video[0]["id"]]), "dmlh and strh count all frames"
    assert out["avih"][4] == len(out["per_segment"][video[0]["id"]][0]), "avih counts the first RIFF chunk's frames"
    assert out["avih"][3] & 0x10, "AVIF_HASINDEX"
    return out


def payloads(data, chunks: list) -> list:
    return [bytes(data[at:at + size]) for at, size in chunks]


def spans(avi: dict) -> list:
    """Bytes every RIFF chunk spans, header included"""
    return [end - begin for begin, end, _ in avi["riffs"]]
