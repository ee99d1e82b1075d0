"""
The PNG stream of csrc/png_kernels.hpp restated in numpy / Python, from the filter choice to the last byte: row filters, the
run-length parse, the code lengths with the header's tie-breaking and length limiter, the block headers, the LSB-first bit packing,
CRC-32, Adler-32 and the chunking. `encode(picture)` gives the bytes the device gives. Nothing here reads the device or zlib: the
tests hold this file against zlib and Pillow (tests/test_host_png.py) and the device against this file (tests/test_gpu_png.py).
"""
from __future__ import annotations

import heapq
import struct

import numpy as np

STRIPE_ROWS = 8
SIGNATURE = b"\x89PNG\r\n\x1a\n"
LITERALS, DISTANCES, SYMBOLS = 286, 30, 316                    # a histogram: 286 literal/length counts, then 30 distance counts
END_OF_BLOCK = 256
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)     # of the code-length code's lengths in a block header
FIXED_LENGTHS = np.array([8]*144 + [9]*112 + [7]*24 + [8]*6 + [5]*30, np.int64)  # RFC 1951 3.2.6, over the 316 symbols


# ---- checksums ---------------------------------------------------------------------------------------------------------------------

def _crc_table():
    table = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ 0xedb88320 if c & 1 else c >> 1
        table.append(c)
    return table


CRC_TABLE = _crc_table()


def crc32(data: bytes) -> int:
    c = 0xffffffff
    for byte in data:
        c = CRC_TABLE[(c ^ byte) & 0xff] ^ (c >> 8)
    return c ^ 0xffffffff


def adler32(data: bytes) -> int:
    values = np.frombuffer(data, np.uint8).astype(np.int64)
    n = len(values)
    a = (1 + int(values.sum())) % 65521
    b = (n + int((values*np.arange(n, 0, -1, dtype=np.int64) % 65521).sum())) % 65521
    return (b << 16) | a


def chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", crc32(kind + data))


# ---- filter --------------------------------------------------------------------------------------------------------------------------

def filter_rows(picture: np.ndarray):
    """(h, w, 3) uint8, top row first → (filtered stream as (h, 3w + 1) uint8, the rows' filter types). Per row the type of None, Sub,
    Up, Average, Paeth whose filtered bytes, read as signed, have the smallest sum of absolute values; ties to the lowest type"""
    h, w = picture.shape[:2]
    raw = picture.reshape(h, 3*w).astype(np.int64)
    out, types = np.zeros((h, 3*w + 1), np.uint8), []
    for y in range(h):
        x = raw[y]
        b = raw[y - 1] if y else np.zeros_like(x)
        a = np.concatenate([np.zeros(3, np.int64), x[:-3]])
        c = np.concatenate([np.zeros(3, np.int64), b[:-3]])
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        candidates = [(x - q) & 0xff for q in (np.zeros_like(x), a, b, (a + b) >> 1, paeth)]
        sums = [int(np.where(f < 128, f, 256 - f).sum()) for f in candidates]
        best = int(np.argmin(sums))                                   # (argmin: the first of equals)
        types.append(best)
        out[y, 0], out[y, 1:] = best, candidates[best]
    return out, types


# ---- parse ---------------------------------------------------------------------------------------------------------------------------

def length_symbol(length: int):
    """A match length 3…258 → (symbol 257…285, extra bits, their value)"""
    if length == 258:
        return 285, 0, 0
    n = length - 3
    if n < 8:
        return 257 + n, 0, 0
    extra = n.bit_length() - 3
    return 261 + 4*extra + ((n >> extra) & 3), extra, n & ((1 << extra) - 1)


def parse(data: bytes):
    """Greedy literals and distance-1 matches of one stripe: [("literal", byte) | ("match", length)]. A match starts where a byte
    repeats the byte before it (of the same stripe) and at least 3 such bytes follow each other; it takes up to 258 of them."""
    tokens, i, n = [], 0, len(data)
    while i < n:
        run = 0
        if i > 0:
            while run < 258 and i + run < n and data[i + run] == data[i - 1]:
                run += 1
        if run >= 3:
            tokens.append(("match", run))
            i += run
        else:
            tokens.append(("literal", data[i]))
            i += 1
    return tokens


def histogram(tokens) -> np.ndarray:
    counts = np.zeros(SYMBOLS, np.int64)
    for kind, value in tokens:
        if kind == "literal":
            counts[value] += 1
        else:
            counts[length_symbol(value)[0]] += 1
            counts[LITERALS] += 1                                      # distance 1 is distance symbol 0
    counts[END_OF_BLOCK] += 1
    return counts


# ---- codes ---------------------------------------------------------------------------------------------------------------------------

def code_lengths(counts, limit: int) -> np.ndarray:
    """Huffman code lengths of one alphabet, as png_kernels.hpp states them:
      * while fewer than two symbols have a count, the lowest-numbered symbol without one gets the count 1;
      * the two nodes with the smallest (weight, index) are merged until one is left — leaves have their symbol as index, the k-th
        node made has index n + k; a symbol's length is its depth;
      * while the deepest symbol is deeper than `limit`, every count w > 0 becomes (w + 1) >> 1 and the tree is built again."""
    weights = [int(c) for c in counts]
    n = len(weights)
    while sum(1 for w in weights if w) < 2:
        weights[next(s for s in range(n) if not weights[s])] = 1
    while True:
        heap = [(w, s) for s, w in enumerate(weights) if w]
        heapq.heapify(heap)
        parent, made = {}, n
        while len(heap) > 1:
            (w1, i1), (w2, i2) = heapq.heappop(heap), heapq.heappop(heap)
            parent[i1] = parent[i2] = made
            heapq.heappush(heap, (w1 + w2, made))
            made += 1
        lengths = np.zeros(n, np.int64)
        for s, w in enumerate(weights):
            node = s
            while w and node in parent:
                node = parent[node]
                lengths[s] += 1
        if lengths.max() <= limit:
            return lengths
        weights = [(w + 1) >> 1 if w else 0 for w in weights]


def canonical(lengths):
    """RFC 1951 3.2.2: → the codes, bit-reversed (they are packed from their most significant bit, everything else LSB first)"""
    lengths = [int(v) for v in lengths]
    count = [0]*17
    for v in lengths:
        count[v] += 1
    count[0] = 0
    code, first = 0, [0]*17
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        first[bits] = code
    codes = []
    for v in lengths:
        if v:
            codes.append(int(format(first[v], f"0{v}b")[::-1], 2))
            first[v] += 1
        else:
            codes.append(0)
    return codes


def tables(counts):
    """The tables step on a 316-entry histogram → (the dynamic code's 316 lengths, whether the block is written with the fixed codes,
    the code-length code's 19 lengths)"""
    counts = np.asarray(counts, np.int64)
    lengths = np.concatenate([code_lengths(counts[:LITERALS], 15), code_lengths(counts[LITERALS:], 15)])
    meta = np.zeros(19, np.int64)
    for v in lengths:
        meta[v] += 1
    meta_lengths = code_lengths(meta, 7)
    extra = sum(int(counts[symbol])*((symbol - 261)//4) for symbol in range(265, 285))     # the length symbols' extra bits
    dynamic = 3 + 14 + 19*3 + int(meta_lengths[lengths].sum()) + int((counts*lengths).sum()) + extra
    fixed = 3 + int((counts*FIXED_LENGTHS).sum()) + extra
    return lengths, not dynamic < fixed, meta_lengths


class Bits:
    def __init__(self):
        self.value, self.count = 0, 0

    def put(self, value: int, bits: int):
        self.value |= value << self.count
        self.count += bits

    def align(self):
        self.count = (self.count + 7) & ~7

    def bytes(self) -> bytes:
        assert self.count % 8 == 0
        return self.value.to_bytes(self.count//8, "little")


def deflate_stripe(data: bytes, out: Bits, last: bool, stats: dict | None = None) -> None:
    """One stripe's block into `out`: dynamic codes of its own, or the fixed ones if those are not longer; every stripe but the last
    ends with an empty stored block on a byte boundary"""
    tokens = parse(data)
    counts = histogram(tokens)
    lengths, fixed, meta_lengths = tables(counts)
    if stats is not None:
        stats.setdefault("fixed", []).append(fixed)
        stats.setdefault("longest_match", []).append(max([v for k, v in tokens if k == "match"], default=0))
    start = out.count
    out.put((1 if last else 0) | ((1 if fixed else 2) << 1), 3)
    if fixed:
        lengths = FIXED_LENGTHS
    else:
        out.put(LITERALS - 257, 5)
        out.put(DISTANCES - 1, 5)
        out.put(19 - 4, 4)
        for symbol in ORDER:
            out.put(int(meta_lengths[symbol]), 3)
        meta_codes = canonical(meta_lengths)
        for v in lengths:
            out.put(meta_codes[v], int(meta_lengths[v]))
    # (the fixed literal/length code is canonical over 288 symbols: 286 and 287 take two of the 8-bit codes and never occur)
    codes = canonical(list(lengths[:LITERALS]) + ([8, 8] if fixed else []))[:LITERALS] + canonical(lengths[LITERALS:])
    for kind, value in tokens:
        if kind == "literal":
            out.put(codes[value], int(lengths[value]))
        else:
            symbol, extra, rest = length_symbol(value)
            out.put(codes[symbol], int(lengths[symbol]))
            out.put(rest, extra)
            out.put(codes[LITERALS], int(lengths[LITERALS]))
    out.put(codes[END_OF_BLOCK], int(lengths[END_OF_BLOCK]))
    if stats is not None:
        stats.setdefault("block_bits", []).append(out.count - start)
    if last:
        out.align()
    else:
        out.put(0, 3)
        out.align()
        out.put(0xffff0000, 32)


def stripes_of(filtered: np.ndarray):
    return [filtered[y:y + STRIPE_ROWS].tobytes() for y in range(0, filtered.shape[0], STRIPE_ROWS)]


def idat_payloads(filtered: np.ndarray, stats: dict | None = None):
    """The data of the IDAT chunks, one per stripe"""
    stripes, payloads = stripes_of(filtered), []
    for k, data in enumerate(stripes):
        out = Bits()
        if k == 0:
            out.put(0x0178, 16)
        last = k == len(stripes) - 1
        deflate_stripe(data, out, last, stats)
        if last:
            out.put(int.from_bytes(struct.pack(">I", adler32(filtered.tobytes())), "little"), 32)
        payloads.append(out.bytes())
    return payloads


def encode(picture: np.ndarray, stats: dict | None = None) -> bytes:
    """(h, w, 3) uint8, top row first → the PNG file"""
    picture = np.ascontiguousarray(picture, np.uint8)
    h, w = picture.shape[:2]
    filtered, types = filter_rows(picture)
    if stats is not None:
        stats["filters"] = types
    body = b"".join(chunk(b"IDAT", data) for data in idat_payloads(filtered, stats))
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + body + chunk(b"IEND", b"")


def capacity(width: int, height: int) -> int:
    """Payload bytes a sink frame is given (sfx_png_capacity): every stripe at its bound ⌈9n/8⌉ + 16, 12 per chunk, 57 for the
    signature, IHDR and IEND, 6 for the zlib header and the Adler-32; rounded up to 16"""
    total = 57 + 6
    for y in range(0, height, STRIPE_ROWS):
        n = min(STRIPE_ROWS, height - y)*(3*width + 1)
        total += (9*n + 7)//8 + 16 + 12
    return (total + 15) & ~15


def chunks(stream: bytes):
    """[(type, data, stored crc)] of a PNG file, and the number of bytes they and the signature take"""
    assert stream[:8] == SIGNATURE
    at, found = 8, []
    while True:
        size, kind = struct.unpack(">I4s", stream[at:at + 8])
        found.append((kind, stream[at + 8:at + 8 + size], struct.unpack(">I", stream[at + 8 + size:at + 12 + size])[0]))
        at += 12 + size
        if kind == b"IEND":
            return found, at


# ---- pictures ------------------------------------------------------------------------------------------------------------------------

KINDS = ("zeros", "horizontal", "vertical", "diagonal", "noise", "ff")


def picture(kind: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    y, x = np.mgrid[0:h, 0:w]
    if kind == "zeros":
        out = np.zeros((h, w, 3), np.int64)
    elif kind == "horizontal":                                        # constant steps along a row: Sub leaves runs
        out = np.stack([x*3, x*5 + 7, 255 - x*2], -1)
    elif kind == "vertical":                                          # every row a shuffle, moved by constant steps from the row above: Up
        base = np.random.default_rng(seed + 1).integers(0, 256, (1, w, 3))
        out = base + np.stack([y*3, y*7, y*11], -1)
    elif kind == "diagonal":                                          # curved in both directions: Average and Paeth
        out = np.stack([(x*x + y*y)//3, (x + 2)*(y + 1), (x*y)//2 + 3*x + 5*y], -1)
    elif kind == "noise":
        out = np.random.default_rng(seed).integers(0, 256, (h, w, 3))
    elif kind == "ff":                                                # rows of 0xFF between noisy ones
        out = np.random.default_rng(seed + 2).integers(250, 256, (h, w, 3))
        out[::2] = 255
    else:
        raise ValueError(kind)
    return (out & 0xff).astype(np.uint8)


SHAPES = [(1, 1), (2, 1), (3, 5), (17, 8), (16, 9), (130, 67), (344, 16)]

FIBONACCI = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765, 10946, 17711, 28657, 46368]


def histograms() -> dict:
    """The four histograms the tables step is pinned on"""
    fibonacci = np.zeros(SYMBOLS, np.int64)
    fibonacci[40:64] = FIBONACCI                                      # 24 literals and nothing else: an unlimited code is 23 bits deep
    single = np.zeros(SYMBOLS, np.int64)
    single[END_OF_BLOCK] = 1
    no_match = np.zeros(SYMBOLS, np.int64)
    no_match[:256] = np.random.default_rng(3).integers(0, 50, 256)
    no_match[END_OF_BLOCK] = 1
    return {"fibonacci": fibonacci, "one-symbol": single, "no-match": no_match, "flat": np.full(SYMBOLS, 7, np.int64)}
