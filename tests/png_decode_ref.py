"""
The PNG decode of csrc/png_decode_kernels.hpp restated in plain Python: inflate with the device's status bits, the segment path's
validation predicate, the Adler-32 check, and the five row filters undone in numpy. Nothing here reads the device. It also holds the
CASE TABLE the host and GPU tests share (tests/test_host_png_in.py holds this file against zlib and Pillow on every case,
tests/test_gpu_png_in.py the device against zlib and Pillow): streams built with zlib, Pillow and tests/png_ref.py.
"""
from __future__ import annotations

import io
import struct
import sys
import zlib
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import png_ref as P  # noqa: E402

BAD_BLOCK, BAD_STORED, BAD_LENGTHS, BAD_CODE, BAD_DISTANCE, OUT_OF_BITS, BAD_SIZE, BAD_FILTER, BAD_ADLER, BAD_DESCRIPTOR = (1 << k for k in range(10))
SERIAL, SEGMENT, LAST_SEGMENT = 0, 1, 2
FLUSH = b"\x00\x00\xff\xff"


class Stop(Exception):
    def __init__(self, bits):
        self.bits = bits


class Reader:
    """Bits of data[begin:end], LSB first, and no others"""

    def __init__(self, data, begin, end):
        self.data, self.at, self.end = data, 8*begin, 8*end

    def peek(self, ahead):
        """The bit `ahead` bits on; 0 behind the end"""
        at = self.at + ahead
        return (self.data[at >> 3] >> (at & 7)) & 1 if at < self.end else 0

    def take(self, count):
        if self.at + count > self.end:
            raise Stop(OUT_OF_BITS)
        value = 0
        for k in range(count):
            value |= ((self.data[(self.at + k) >> 3] >> ((self.at + k) & 7)) & 1) << k
        self.at += count
        return value

    @property
    def left(self):
        return self.end - self.at


def build(lengths):
    """{(length, code): symbol} of the canonical code, or Stop(BAD_LENGTHS) when it is over-subscribed. An incomplete code is kept:
    its missing codes are found when met."""
    count = [0]*16
    for v in lengths:
        count[v] += 1
    count[0], left = 0, 1
    for bits in range(1, 16):
        left = 2*left - count[bits]
        if left < 0:
            raise Stop(BAD_LENGTHS)
    code, first = 0, [0]*16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        first[bits] = code
    table = {}
    for symbol, v in enumerate(lengths):
        if v:
            table[(v, first[v])] = symbol
            first[v] += 1
    return table


FAST_BITS = 10


def symbol_of(reader, table):
    """The next symbol, with the device's rule for which error a bad tail is: the next FAST_BITS bits are looked at together, zeros
    standing in behind the end. A code of up to FAST_BITS bits that begins there is taken, or OUT_OF_BITS when it is longer than
    what is left. Where a longer code begins, bits are taken one by one: OUT_OF_BITS when they run out, BAD_CODE when 15 match
    none. Where no code begins: OUT_OF_BITS with fewer than FAST_BITS bits left, BAD_CODE otherwise."""
    left, code = reader.left, 0
    for length in range(1, 16):
        if length > FAST_BITS and length > left:
            raise Stop(OUT_OF_BITS)
        code = (code << 1) | reader.peek(length - 1)
        if (length, code) in table:
            if length > left:
                raise Stop(OUT_OF_BITS)
            reader.at += length
            return table[(length, code)]
        if length == FAST_BITS and not any(size > FAST_BITS and value >> (size - FAST_BITS) == code for size, value in table):
            raise Stop(OUT_OF_BITS if left < FAST_BITS else BAD_CODE)
    raise Stop(BAD_CODE)


FIXED = (build([8]*144 + [9]*112 + [7]*24 + [8]*8), build([5]*30))


def inflate(data: bytes, begin: int, end: int, limit: int, rule: int = SERIAL):
    """→ (status, output, valid): section 1 of the kernels' header comment. `valid` is the segment path's predicate (rules SEGMENT and
    LAST_SEGMENT); under SERIAL the status carries BAD_SIZE and BAD_ADLER (bytes between the last block and the trailer)."""
    reader, out, final = Reader(data, begin, end), bytearray(), False
    try:
        while True:
            if rule != SERIAL and reader.left == 0:
                break
            header = reader.take(3)
            final, kind = bool(header & 1), header >> 1
            if kind == 3:
                raise Stop(BAD_BLOCK)
            if kind == 0:
                reader.at = (reader.at + 7) & ~7
                length, complement = reader.take(16), reader.take(16)
                if length ^ complement != 0xffff:
                    raise Stop(BAD_STORED)
                if 8*length > reader.left:
                    raise Stop(OUT_OF_BITS)
                if length > limit - len(out):
                    raise Stop(BAD_SIZE)
                out += data[reader.at >> 3:(reader.at >> 3) + length]
                reader.at += 8*length
            else:
                if kind == 1:
                    literal, distance = FIXED
                else:
                    hlit, hdist, hclen = reader.take(5) + 257, reader.take(5) + 1, reader.take(4) + 4
                    if hlit > 286 or hdist > 30:
                        raise Stop(BAD_LENGTHS)
                    meta = [0]*19
                    for k in range(hclen):
                        meta[P.ORDER[k]] = reader.take(3)
                    meta, lengths = build(meta), []
                    while len(lengths) < hlit + hdist:
                        symbol = symbol_of(reader, meta)
                        if symbol < 16:
                            lengths.append(symbol)
                            continue
                        if symbol == 16:
                            if not lengths:
                                raise Stop(BAD_LENGTHS)
                            value, repeat = lengths[-1], 3 + reader.take(2)
                        else:
                            value, repeat = 0, (3 + reader.take(3)) if symbol == 17 else (11 + reader.take(7))
                        if len(lengths) + repeat > hlit + hdist:
                            raise Stop(BAD_LENGTHS)
                        lengths += [value]*repeat
                    if lengths[256] == 0:
                        raise Stop(BAD_LENGTHS)
                    distance, literal = build(lengths[hlit:]), build(lengths[:hlit])
                while True:
                    symbol = symbol_of(reader, literal)
                    if symbol < 256:
                        if len(out) >= limit:
                            raise Stop(BAD_SIZE)
                        out.append(symbol)
                    elif symbol == 256:
                        break
                    else:
                        if symbol > 285:
                            raise Stop(BAD_CODE)
                        s = symbol - 257
                        if s < 8:
                            length = 3 + s
                        elif s == 28:
                            length = 258
                        else:
                            extra = (s >> 2) - 1
                            length = 3 + ((4 + (s & 3)) << extra) + reader.take(extra)
                        d = symbol_of(reader, distance)
                        if d > 29:
                            raise Stop(BAD_CODE)
                        if d < 4:
                            far = 1 + d
                        else:
                            extra = (d >> 1) - 1
                            far = 1 + ((2 + (d & 1)) << extra) + reader.take(extra)
                        if far > len(out):
                            raise Stop(BAD_DISTANCE)
                        if length > limit - len(out):
                            raise Stop(BAD_SIZE)
                        for _ in range(length):
                            out.append(out[-far])
            if final:
                break
    except Stop as stop:
        return stop.bits, bytes(out), False
    pad = -reader.at & 7
    zero_pad = reader.take(pad) == 0 if pad else True
    at_end = reader.left == 0
    if rule == SERIAL:
        status = BAD_SIZE if len(out) != limit else (0 if at_end else BAD_ADLER)
        return status, bytes(out), False
    if rule == LAST_SEGMENT:
        return 0, bytes(out), final and zero_pad and at_end
    return 0, bytes(out), (not final) and pad == 0 and at_end


def unfilter(filtered: np.ndarray, width: int) -> np.ndarray:
    """(height, 1 + 3 width) uint8 → (height, width, 3): Recon of the five filter types, bpp = 3"""
    height = filtered.shape[0]
    out = np.zeros((height, 3*width), np.int64)
    for y in range(height):
        kind, line = int(filtered[y, 0]), filtered[y, 1:].astype(np.int64)
        above = out[y - 1] if y else np.zeros(3*width, np.int64)
        if kind == 0:
            out[y] = line
        elif kind == 2:
            out[y] = (line + above) & 255
        else:
            row = out[y]
            for x in range(3*width):
                a = row[x - 3] if x >= 3 else 0
                b = above[x]
                c = above[x - 3] if x >= 3 else 0
                if kind == 1:
                    predicted = a
                elif kind == 3:
                    predicted = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    predicted = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                row[x] = (line[x] + predicted) & 255
    return out.astype(np.uint8).reshape(height, width, 3)


def split(stream: bytes):
    """A PNG file → (width, height, payload, segment starts, the trailer's Adler-32): what pngsource.stage puts into a staged frame"""
    found, _ = P.chunks(stream)
    width, height = struct.unpack(">II", found[0][1][:8])
    idats = [data for kind, data, _ in found if kind == b"IDAT"]
    joined = b"".join(idats)
    starts, at = [], -2
    for data in idats:
        starts.append(min(max(at, 0), len(joined) - 6))
        at += len(data)
    return width, height, joined[2:-4], starts, struct.unpack(">I", joined[-4:])[0]


def segment_rule(payload: bytes, starts) -> bool:
    """The production rule: at least two segments, every one but the last ending in 00 00 FF FF"""
    return len(starts) >= 2 and all(end >= 4 and payload[end - 4:end] == FLUSH for end in starts[1:])


def decode(stream: bytes, segments=None) -> dict:
    """The whole decode as the device does it → {"status", "filtered" (bytes the inflate produced), "rgb" or None, "info"}"""
    width, height, payload, starts, adler = split(stream)
    expected = height*(1 + 3*width)
    chosen = segment_rule(payload, starts) if segments is None else segments
    info = {"segments": len(starts), "parallel": 0, "fell_back": 0}
    status = out = None
    if chosen:
        ends = starts[1:] + [len(payload)]
        parts = [inflate(payload, begin, end, expected, LAST_SEGMENT if k == len(starts) - 1 else SEGMENT) for k, (begin, end) in enumerate(zip(starts, ends))]
        if all(valid for _, _, valid in parts) and sum(len(part) for _, part, _ in parts) == expected:
            status, out, info["parallel"] = 0, b"".join(part for _, part, _ in parts), 1
        else:
            info["fell_back"] = 1
    if out is None:
        status, out, _ = inflate(payload, 0, len(payload), expected, SERIAL)
    rgb = None
    if not status:
        filtered = np.frombuffer(out, np.uint8).reshape(height, 1 + 3*width)
        if (filtered[:, 0] > 4).any():
            status |= BAD_FILTER
        if P.adler32(out) != adler:
            status |= BAD_ADLER
        if not status:
            rgb = unfilter(filtered, width)
    return {"status": status, "filtered": out, "rgb": rgb, "info": info}


# ---- building streams ------------------------------------------------------------------------------------------------------------------

def png(width: int, height: int, idats) -> bytes:
    return P.SIGNATURE + P.chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)) + b"".join(P.chunk(b"IDAT", data) for data in idats) + P.chunk(b"IEND", b"")


def zlib_stream(raw: bytes, filtered: bytes) -> bytes:
    """A raw deflate stream in the zlib wrapper"""
    return b"\x78\x01" + raw + struct.pack(">I", zlib.adler32(filtered))


def filtered_of(picture: np.ndarray, types=None) -> np.ndarray:
    """The filtered stream of a picture with the row's filter types given (None: png_ref's own choice)"""
    if types is None:
        return P.filter_rows(picture)[0]
    h, w = picture.shape[:2]
    raw = picture.reshape(h, 3*w).astype(np.int64)
    out = np.zeros((h, 3*w + 1), np.uint8)
    for y in range(h):
        x = raw[y]
        b = raw[y - 1] if y else np.zeros_like(x)
        a = np.concatenate([np.zeros(3, np.int64), x[:-3]])
        c = np.concatenate([np.zeros(3, np.int64), b[:-3]])
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        out[y, 0] = types[y]
        out[y, 1:] = (x - (0, a, b, (a + b) >> 1, paeth)[types[y]]) & 255
    return out


def deflated(filtered: np.ndarray, level=6, strategy=zlib.Z_DEFAULT_STRATEGY) -> bytes:
    """The PNG file of a filtered stream, one IDAT, written by zlib"""
    packer = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return png((filtered.shape[1] - 1)//3, filtered.shape[0], [packer.compress(filtered.tobytes()) + packer.flush()])


def pillow(picture: np.ndarray, level: int) -> bytes:
    from PIL import Image
    out = io.BytesIO()
    Image.fromarray(picture, "RGB").save(out, "PNG", compress_level=level)
    return out.getvalue()


def distance_symbol(distance: int):
    if distance <= 4:
        return distance - 1, 0, 0
    extra = (distance - 1).bit_length() - 2
    return 2*extra + 2 + (((distance - 1) >> extra) & 1), extra, (distance - 1) & ((1 << extra) - 1)


def block(tokens, final: bool, out: P.Bits, lengths=None, distances=None) -> None:
    """One block of ("literal", byte) / ("match", length, distance) tokens into `out`: fixed codes, or dynamic ones with the given
    literal/length and distance code lengths (the header spells every length out: no repeat symbols)"""
    if lengths is None:
        out.put((1 if final else 0) | 2, 3)
        lengths, distances = [int(v) for v in P.FIXED_LENGTHS[:P.LITERALS]] + [8, 8], [5]*30
    else:
        lengths, distances = [int(v) for v in lengths], [int(v) for v in distances]
        out.put((1 if final else 0) | 4, 3)
        out.put(len(lengths) - 257, 5)
        out.put(len(distances) - 1, 5)
        out.put(15, 4)
        meta = np.zeros(19, np.int64)
        for v in lengths + distances:
            meta[v] += 1
        meta_lengths = P.code_lengths(meta, 7)
        for symbol in P.ORDER:
            out.put(int(meta_lengths[symbol]), 3)
        meta_codes = P.canonical(meta_lengths)
        for v in lengths + distances:
            out.put(meta_codes[v], int(meta_lengths[v]))
    codes, far = P.canonical(lengths), P.canonical(distances)
    for token in tokens:
        if token[0] == "literal":
            out.put(codes[token[1]], lengths[token[1]])
        elif token[0] == "symbol":                                    # a literal/length symbol as it stands (damage cases)
            out.put(codes[token[1]], lengths[token[1]])
        else:
            symbol, extra, rest = P.length_symbol(token[1])
            out.put(codes[symbol], lengths[symbol])
            out.put(rest, extra)
            symbol, extra, rest = distance_symbol(token[2])
            out.put(far[symbol], distances[symbol])
            out.put(rest, extra)
    out.put(codes[256], lengths[256])


def hand(width: int, height: int, filtered: bytes, blocks) -> bytes:
    """A PNG file whose deflate stream is the given blocks [(tokens, lengths, distances)]"""
    out = P.Bits()
    for k, (tokens, lengths, distances) in enumerate(blocks):
        block(tokens, k == len(blocks) - 1, out, lengths, distances)
    out.align()
    return png(width, height, [zlib_stream(out.bytes(), filtered)])


def expand(tokens) -> bytes:
    out = bytearray()
    for token in tokens:
        if token[0] == "literal":
            out.append(token[1])
        else:
            for _ in range(token[1]):
                out.append(out[-token[2]])
    return bytes(out)


def literals(data: bytes):
    return [("literal", v) for v in data]


# ---- the case table --------------------------------------------------------------------------------------------------------------------

PICTURE_SHAPES = [(1, 1), (7, 1), (1, 7), (37, 21), (21, 9), (85, 9), (86, 9), (40, 63), (40, 64), (40, 65), (86, 129)]
_cases: dict = {}


def mixed(w: int, h: int, seed: int = 0) -> np.ndarray:
    """Smooth in places, noisy in others: every filter type is chosen somewhere and matches occur"""
    picture = P.picture("diagonal", w, h)
    noise = P.picture("noise", w, h, seed)
    picture[::3] = noise[::3] >> 5
    picture[:, : w//3] = P.picture("horizontal", w, h)[:, : w//3]
    return picture


def cases() -> dict:
    """name → {"stream": the PNG file, "paths": which of (False, True) — the serial path, the segment path — the case is decoded on}.
    Built once."""
    if _cases:
        return _cases
    add = lambda name, stream, paths=(False, True): _cases.__setitem__(name, {"stream": stream, "paths": paths})     # noqa: E731
    # pictures: this project's stream (a segment per stripe of 8 rows) and zlib's (one segment)
    for w, h in PICTURE_SHAPES:
        add(f"own-{w}x{h}", P.encode(mixed(w, h)))
        add(f"zlib-{w}x{h}", deflated(filtered_of(mixed(w, h, 1))), (False,))
    for kind in P.KINDS:
        add(f"own-{kind}", P.encode(P.picture(kind, 37, 21)))
    for kind in range(5):                                             # each filter type in row 0, in a stripe's first row and in a band's first row
        types = [(kind + y) % 5 for y in range(66)]
        types[0] = types[8] = types[64] = kind
        add(f"filter-{kind}", deflated(filtered_of(mixed(24, 66, kind), types)), (False,))
    add("all-paeth", deflated(filtered_of(mixed(33, 70, 7), [4]*70)), (False,))
    # streams
    big = P.picture("noise", 200, 110)                                # 66 110 bytes of filtered stream: a stored block of 65 535 bytes fits
    stored = zlib.compressobj(0, zlib.DEFLATED, 15)
    data = filtered_of(big, [0]*110).tobytes()
    add("stored", png(200, 110, [stored.compress(data[:100]) + stored.flush(zlib.Z_SYNC_FLUSH) + stored.compress(data[100:]) + stored.flush()]), (False,))
    small = filtered_of(mixed(37, 21, 3))
    for name, level, strategy in (("fixed", 6, zlib.Z_FIXED), ("huffman-only", 6, zlib.Z_HUFFMAN_ONLY), ("rle", 6, zlib.Z_RLE), ("level-9", 9, zlib.Z_DEFAULT_STRATEGY)):
        add(name, deflated(small, level, strategy), (False,))
    add("level-9-flat", deflated(filtered_of(P.picture("horizontal", 86, 129)), 9), (False,))      # long repeats: symbols 16, 17, 18; short HLIT and HDIST
    stats: dict = {}
    # tall and narrow: 138 segments (the scan's carry across groups of 64), 18 bands in 3 rounds of the unfilter's 8 waves; and wide:
    # 813 steps a band, 26 chunks, more than the 24 a round is apart at the least
    add("own-8x1100", P.encode(mixed(8, 1100, 11)))
    add("zlib-3000x3", deflated(filtered_of(mixed(3000, 3, 12), [4, 3, 1])), (False,))
    add("own-fixed-stripe", P.encode(P.picture("noise", 2, 20), stats))
    assert any(stats["fixed"]) and len(stats["fixed"]) == 3
    for level in (0, 1, 9):
        add(f"pillow-{level}", pillow(big if level == 0 else mixed(86, 129, 5), level), (False,))
    zeros = bytes(4*(1 + 3*86))
    add("match-258-distance-1", hand(86, 4, zeros, [([("literal", 0)] + [("match", 258, 1)]*4 + literals(zeros[1033:]), None, None)]))
    far = bytearray(filtered_of(mixed(86, 129, 9)).tobytes())
    far[32768:32868] = far[:100]                                      # (no filter byte lies in 32768…32867: row 127 starts at 32893)
    add("distance-32768", hand(86, 129, bytes(far), [(literals(far[:32768]) + [("match", 100, 32768)] + literals(far[32868:]), None, None)]))
    tokens = literals(bytes(range(6))) + [("match", 10, 6)] + literals(bytes([9, 8, 7, 6, 5, 4]))    # 7 x 1: the filter byte 0 and 21 more; the match overlaps itself
    add("match-to-the-first-byte", hand(7, 1, expand(tokens), [(tokens, None, None)]))
    # a dynamic block whose only distance code has one bit; and one with 15-bit codes
    tokens = [("literal", 0)] + [("match", 258, 1)]*4 + literals(zeros[1033:])
    counts = np.zeros(286, np.int64)
    counts[0], counts[256], counts[285] = len(zeros) - 1033 + 1, 1, 4
    add("one-bit-distance-code", hand(86, 4, zeros, [(tokens, P.code_lengths(counts, 15), [1])]))
    counts = np.zeros(286, np.int64)                                  # the Fibonacci histogram's first 16 counts: a code 15 bits deep without the limiter
    fibonacci = P.histograms()["fibonacci"][40:56]
    counts[256], counts[0], counts[41:55] = fibonacci[0], fibonacci[1], fibonacci[2:]      # (the filter byte 0 must have a code, and the block its end)
    deep = P.code_lengths(counts, 15)
    assert deep.max() == 15
    line = bytes([0]) + bytes(41 + (k*5) % 14 for k in range(3*23))
    add("15-bit-codes", hand(23, 1, line, [(literals(line), deep, [0])]))
    # paths: cuts at IDAT boundaries
    rows = filtered_of(mixed(37, 21, 4))
    for name, flush in (("full-flush", zlib.Z_FULL_FLUSH), ("sync-flush", zlib.Z_SYNC_FLUSH)):
        packer = zlib.compressobj(9, zlib.DEFLATED, 15)
        repeated = np.concatenate([rows[:7]]*3)                       # 21 rows, the same 7 three times: level 9 reaches back across a cut
        idats = [packer.compress(repeated[y:y + 7].tobytes()) + packer.flush(flush) for y in (0, 7)] + [packer.compress(repeated[14:].tobytes()) + packer.flush()]
        add(name, png(37, 21, idats))
    try:
        zlib.decompressobj(-15).decompress(P.chunks(_cases["sync-flush"]["stream"])[0][2][1])
        raise AssertionError("the sync-flush case holds no back reference across its cut")
    except zlib.error:
        pass
    whole = P.chunks(_cases["pillow-0"]["stream"])[0]
    assert sum(1 for kind, _, _ in whole if kind == b"IDAT") >= 2
    _cases["pillow-0"]["paths"] = (False, True)
    # a stored block that CONTAINS 00 00 FF FF, and the IDAT cut right behind those bytes
    trap = np.zeros((3, 5, 3), np.uint8)
    trap[1, 1:] = 255
    data = filtered_of(trap, [0, 0, 0]).tobytes()
    stream = zlib.compress(data, 0)
    cut = stream.index(FLUSH, 7) + 4
    add("flush-bytes-in-a-stored-block", png(5, 3, [stream[:cut], stream[cut:]]))
    return _cases


PARALLEL = ("own-37x21", "own-86x129", "own-8x1100", "own-fixed-stripe", "full-flush")
FELL_BACK = ("sync-flush", "pillow-0", "flush-bytes-in-a-stored-block")


def damaged() -> dict:
    """name → (the PNG file, the status bit the decode must set): one per bit the kernels can set from a stream"""
    width, height = 5, 3
    good = filtered_of(mixed(width, height, 2), [0, 1, 4])
    data = good.tobytes()
    out = {}

    def raw(bits: P.Bits) -> bytes:
        bits.align()
        return png(width, height, [zlib_stream(bits.bytes(), data)])
    bits = P.Bits()
    bits.put(1 | (3 << 1), 3)
    out["block-type-3"] = (raw(bits), BAD_BLOCK)
    bits = P.Bits()
    bits.put(1, 3)
    bits.align()
    bits.put(len(data), 16)
    bits.put(len(data), 16)                                           # not the complement
    out["stored-complement"] = (png(width, height, [zlib_stream(bits.bytes() + data, data)]), BAD_STORED)
    bits = P.Bits()
    bits.put(1 | 4, 3)
    bits.put(0, 5); bits.put(0, 5); bits.put(15, 4)                   # noqa: E702
    for _ in range(19):
        bits.put(1, 3)                                                # nineteen codes of one bit
    out["over-subscribed"] = (raw(bits), BAD_LENGTHS)
    bits = P.Bits()
    block(literals(data[:4]) + [("symbol", 286)], True, bits)
    out["reserved-symbol"] = (raw(bits), BAD_CODE)
    bits = P.Bits()
    block(literals(data[:1]) + [("match", 3, 5)] + literals(data[4:]), True, bits)
    out["distance-too-far"] = (raw(bits), BAD_DISTANCE)
    whole = zlib.compress(data, 6)
    out["cut-short"] = (png(width, height, [whole[:2 + (len(whole) - 6)//2] + whole[-4:]]), OUT_OF_BITS)
    longer = data + data[-16:]
    out["a-row-too-many"] = (png(width, height, [zlib.compress(longer, 6)]), BAD_SIZE)
    shorter = data[:-16]
    out["a-row-missing"] = (png(width, height, [zlib.compress(shorter, 6)]), BAD_SIZE)
    wrong = bytearray(data)
    wrong[16] = 7
    out["filter-type-7"] = (png(width, height, [zlib.compress(bytes(wrong), 6)]), BAD_FILTER)
    out["adler"] = (png(width, height, [whole[:-1] + bytes([whole[-1] ^ 1])]), BAD_ADLER)
    return out
