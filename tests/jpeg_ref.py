"""
The project's Motion-JPEG stream restated in numpy / float64 (csrc/jpeg_kernels.hpp holds the definition): colour, chroma mean,
padding, DCT, quantisation, the Annex K tables, Huffman coding with one restart interval per MCU row — an encoder, and a decoder
that stops at the quantised coefficients (any baseline JPEG with interleaved scans: it reads the file's own tables).

Coefficients travel as int arrays of shape (mcu rows, mcus per row, 6, 64): Y0 Y1 Y2 Y3 Cb Cr per MCU, zigzag order.
"""
from __future__ import annotations

import struct

import numpy as np

LUMINANCE = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
CHROMINANCE = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99]*32)

DC_LUMINANCE = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMINANCE = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMINANCE = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMINANCE = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))


def zigzag_order() -> np.ndarray:
    """natural index of each zigzag position"""
    order = sorted(range(64), key=lambda k: (k//8 + k % 8, (k//8 if (k//8 + k % 8) % 2 else k % 8)))
    return np.array(order)


ZIGZAG = zigzag_order()
DCT = np.array([[(np.sqrt(0.125) if u == 0 else 0.5)*np.cos((2*x + 1)*u*np.pi/16) for x in range(8)] for u in range(8)])


def quant_tables(quality: int) -> tuple[np.ndarray, np.ndarray]:
    """(luminance, chrominance) in natural order: the usual scaling of the Annex K tables"""
    if not 1 <= quality <= 100:
        raise ValueError(f"jpeg_quality {quality}: 1 to 100")
    scale = 5000//quality if quality < 50 else 200 - 2*quality
    return tuple(np.clip((base*scale + 50)//100, 1, 255) for base in (LUMINANCE, CHROMINANCE))


def huffman_codes(bits, values) -> dict[int, tuple[int, int]]:
    """symbol → (code, length), the standard's Annex C procedure"""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[values[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def padded(rgb: np.ndarray) -> np.ndarray:
    """whole 16 x 16 MCUs by repeating the last column and the last row"""
    h, w = rgb.shape[:2]
    return np.pad(rgb, ((0, -h % 16), (0, -w % 16), (0, 0)), mode="edge")


def planes(rgb: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Y (Hp x Wp), Cb and Cr (Hp/2 x Wp/2) of a top-down RGB8 picture, integers 0…255"""
    p = padded(rgb).astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = np.clip((77*r + 150*g + 29*b + 128) >> 8, 0, 255)
    mean = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2
    r, g, b = mean[..., 0], mean[..., 1], mean[..., 2]
    cb = np.clip(((-43*r - 85*g + 128*b + 128) >> 8) + 128, 0, 255)
    cr = np.clip(((128*r - 107*g - 21*b + 128) >> 8) + 128, 0, 255)
    return y, cb, cr


def blocks_of(plane: np.ndarray) -> np.ndarray:
    """(rows of blocks, blocks per row, 8, 8)"""
    h, w = plane.shape
    return plane.reshape(h//8, 8, w//8, 8).transpose(0, 2, 1, 3)


def scaled_coefficients(rgb: np.ndarray, quality: int) -> np.ndarray:
    """c/q in float64, in front of the rounding: (mcu rows, mcus per row, 6, 64) in zigzag order"""
    y, cb, cr = planes(rgb)
    tables = quant_tables(quality)
    out = np.empty((y.shape[0]//16, y.shape[1]//16, 6, 64))

    def transform(plane, table):
        b = blocks_of(plane.astype(np.float64) - 128.0)
        c = np.einsum("vy,ijyx,ux->ijvu", DCT, b, DCT)
        return (c.reshape(*c.shape[:2], 64)/table)[..., ZIGZAG]

    luma = transform(y, tables[0])
    for k in range(4):
        out[:, :, k] = luma[k//2::2, k % 2::2]
    out[:, :, 4] = transform(cb, tables[1])
    out[:, :, 5] = transform(cr, tables[1])
    return out


def round_half_away(x: np.ndarray) -> np.ndarray:
    return (np.sign(x)*np.floor(np.abs(x) + 0.5)).astype(np.int64)


def coefficients(rgb: np.ndarray, quality: int) -> np.ndarray:
    q = round_half_away(scaled_coefficients(rgb, quality))
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    return q


def tie_distance(rgb: np.ndarray, quality: int) -> np.ndarray:
    """how far each value in front of the rounding is from a tie (…, -0.5, 0.5, 1.5, …)"""
    s = np.abs(scaled_coefficients(rgb, quality))
    return np.abs(s - np.floor(s) - 0.5)


# ---- the stream --------------------------------------------------------------------------------------------------------------------

def header(width: int, height: int, quality: int) -> bytes:
    """SOI, APP0, two DQT, SOF0, four DHT, DRI, SOS: everything in front of the entropy-coded data"""
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xe0" + struct.pack(">H5sBBBHHBB", 16, b"JFIF\0", 1, 1, 0, 1, 1, 0, 0)
    for index, table in enumerate(quant_tables(quality)):
        out += b"\xff\xdb" + struct.pack(">HB", 67, index) + bytes(int(v) for v in table[ZIGZAG])
    out += b"\xff\xc0" + struct.pack(">HBHHB", 17, 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for selector, (bits, values) in ((0x00, DC_LUMINANCE), (0x10, AC_LUMINANCE), (0x01, DC_CHROMINANCE), (0x11, AC_CHROMINANCE)):
        out += b"\xff\xc4" + struct.pack(">HB", 19 + len(values), selector) + bytes(bits) + bytes(values)
    out += b"\xff\xdd" + struct.pack(">HH", 4, (width + 15)//16)
    out += b"\xff\xda" + struct.pack(">HB", 12, 3) + bytes([1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return bytes(out)


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code: int, length: int) -> None:
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xff
            self.out.append(byte)
            if byte == 0xff:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self) -> bytes:
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        data, self.out = bytes(self.out), bytearray()
        return data


def encode_interval(row: np.ndarray, stats: dict | None = None) -> bytes:
    """One MCU row of coefficients (mcus, 6, 64) → its entropy-coded segment (stuffed, padded with ones)"""
    dc = (huffman_codes(*DC_LUMINANCE), huffman_codes(*DC_CHROMINANCE))
    ac = (huffman_codes(*AC_LUMINANCE), huffman_codes(*AC_CHROMINANCE))
    writer, predictor = BitWriter(), [0, 0, 0]
    for mcu in row:
        for b, block in enumerate(mcu):
            component = 0 if b < 4 else b - 3
            table = 1 if component else 0
            diff = int(block[0]) - predictor[component]
            predictor[component] = int(block[0])
            size = abs(diff).bit_length()
            if stats is not None:
                stats["dc_size"] = max(stats.get("dc_size", 0), size)
            writer.put(*dc[table][size])
            if size:
                writer.put((diff if diff >= 0 else diff - 1) & ((1 << size) - 1), size)
            run = 0
            for k in range(1, 64):
                value = int(block[k])
                if value == 0:
                    run += 1
                    continue
                while run >= 16:
                    writer.put(*ac[table][0xf0])
                    run -= 16
                    if stats is not None:
                        stats["zrl"] = stats.get("zrl", 0) + 1
                size = abs(value).bit_length()
                writer.put(*ac[table][(run << 4) | size])
                writer.put((value if value >= 0 else value - 1) & ((1 << size) - 1), size)
                run = 0
            if run:
                writer.put(*ac[table][0x00])
    return writer.flush()


def encode_coefficients(q: np.ndarray, width: int, height: int, quality: int, stats: dict | None = None, prefix: bytes | None = None,
                        interval: int | None = None) -> bytes:
    """`prefix`: another header than this definition's (a file's own, up to and including SOS); `interval`: MCUs per restart interval
    when it is not the MCU row"""
    out = bytearray(header(width, height, quality) if prefix is None else prefix)
    if interval:
        flat = q.reshape(-1, *q.shape[2:])
        q = [flat[k:k + interval] for k in range(0, len(flat), interval)]
    for index, row in enumerate(q):
        if index:
            out += bytes([0xff, 0xd0 + (index - 1) % 8])
        out += encode_interval(row, stats)
    return bytes(out + b"\xff\xd9")


def encode(rgb: np.ndarray, quality: int = 90, stats: dict | None = None) -> bytes:
    """A top-down RGB8 picture (h, w, 3) → the baseline JFIF stream of the definition"""
    return encode_coefficients(coefficients(rgb, quality), rgb.shape[1], rgb.shape[0], quality, stats)


# ---- decoder, down to the quantised coefficients -------------------------------------------------------------------------------------

class BitReader:
    def __init__(self, data: bytes):
        self.data, self.pos, self.acc, self.n = data, 0, 0, 0

    def bit(self) -> int:
        if self.n == 0:
            byte = self.data[self.pos]
            self.pos += 1
            if byte == 0xff:
                assert self.data[self.pos] == 0, "marker inside entropy-coded data"
                self.pos += 1
            self.acc, self.n = byte, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, count: int) -> int:
        value = 0
        for _ in range(count):
            value = (value << 1) | self.bit()
        return value

    def symbol(self, lookup: dict) -> int:
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (code, length) in lookup:
                return lookup[(code, length)]
        raise ValueError("no Huffman code matches")

    def align(self) -> None:
        self.n = 0


def extend(value: int, size: int) -> int:
    return value if size == 0 or value >= (1 << (size - 1)) else value - (1 << size) + 1


def decode(stream: bytes) -> dict:
    """A baseline JPEG (one interleaved scan) → {"width", "height", "sampling", "quant" (natural order, by table), "restart_interval",
    "restart_markers" (the n of every RSTn met, in order), "coefficients": (mcu rows, mcus per row, blocks per MCU, 64) in zigzag order,
    "tables": {(class, id): (bits, values)}}"""
    assert stream[:2] == b"\xff\xd8", "no SOI"
    pos, info = 2, {"quant": {}, "tables": {}, "restart_interval": 0, "restart_markers": []}
    lookups, components = {}, []
    while True:
        assert stream[pos] == 0xff, f"marker expected at {pos}"
        marker = stream[pos + 1]
        length = struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        body = stream[pos + 4:pos + 2 + length]
        pos += 2 + length
        if marker == 0xdb:
            while body:
                assert body[0] >> 4 == 0, "16-bit quantisation table"
                table = np.zeros(64, np.int64)
                table[ZIGZAG] = list(body[1:65])
                info["quant"][body[0] & 15] = table
                body = body[65:]
        elif marker == 0xc0:
            precision, info["height"], info["width"], count = struct.unpack(">BHHB", body[:6])
            assert precision == 8
            components = [(body[6 + 3*k], body[7 + 3*k] >> 4, body[7 + 3*k] & 15, body[8 + 3*k]) for k in range(count)]
            info["sampling"] = [(h, v) for _, h, v, _ in components]
        elif marker in (0xc1, 0xc2, 0xc3, 0xc9, 0xca):
            raise ValueError("not a baseline JPEG")
        elif marker == 0xc4:
            while body:
                bits, total = list(body[1:17]), sum(body[1:17])
                values = list(body[17:17 + total])
                info["tables"][(body[0] >> 4, body[0] & 15)] = (bits, values)
                lookups[(body[0] >> 4, body[0] & 15)] = {pair: symbol for symbol, pair in huffman_codes(bits, values).items()}
                body = body[17 + total:]
        elif marker == 0xdd:
            info["restart_interval"] = struct.unpack(">H", body[:2])[0]
        elif marker == 0xda:
            selectors = {body[1 + 2*k]: (body[2 + 2*k] >> 4, body[2 + 2*k] & 15) for k in range(body[0])}
            break
    hmax, vmax = max(h for _, h, _, _ in components), max(v for _, _, v, _ in components)
    mcus_x, mcus_y = -(-info["width"]//(8*hmax)), -(-info["height"]//(8*vmax))
    layout = [(index, selectors[cid]) for index, (cid, h, v, _) in enumerate(components) for _ in range(h*v)]
    out = np.zeros((mcus_y, mcus_x, len(layout), 64), np.int64)
    reader, predictor = BitReader(stream[pos:]), [0]*len(components)
    for n in range(mcus_x*mcus_y):
        if info["restart_interval"] and n and n % info["restart_interval"] == 0:
            reader.align()
            marker = reader.data[reader.pos:reader.pos + 2]
            assert marker[0] == 0xff and 0xd0 <= marker[1] <= 0xd7, f"RSTn expected before MCU {n}, found {marker.hex()}"
            info["restart_markers"].append(marker[1] - 0xd0)
            reader.pos += 2
            predictor = [0]*len(components)
        for b, (component, (dc_table, ac_table)) in enumerate(layout):
            block = out[n//mcus_x, n % mcus_x, b]
            size = reader.symbol(lookups[(0, dc_table)])
            predictor[component] += extend(reader.bits(size), size)
            block[0] = predictor[component]
            k = 1
            while k < 64:
                symbol = reader.symbol(lookups[(1, ac_table)])
                run, size = symbol >> 4, symbol & 15
                if size == 0:
                    if run != 15:
                        break
                    k += 16
                    continue
                k += run
                block[k] = extend(reader.bits(size), size)
                k += 1
    reader.align()
    assert reader.data[reader.pos:reader.pos + 2] == b"\xff\xd9", "EOI expected behind the last MCU"
    info["coefficients"] = out
    info["length"] = pos + reader.pos + 2
    return info


def picture(kind: str, width: int, height: int, seed: int = 0) -> np.ndarray:
    """The test pictures, top-down RGB8: "gradient", seeded "noise", an 8 x 8 black-and-white "checker", flat "grey", "extremes" (noise
    whose first two 8 x 8 blocks are black and white: a DC difference of 11 bits at quality 100) and "sparse" (grey blocks that each carry
    one high-frequency cosine: long zero runs)"""
    y, x = np.mgrid[0:height, 0:width]
    if kind == "gradient":
        return np.stack([(x*5 + y) % 256, (y*7 + 3) % 256, (x*2 + y*3) % 256], -1).astype(np.uint8)
    if kind in ("noise", "extremes"):
        out = np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)
        if kind == "extremes":
            out[:8, :8], out[:8, 8:16] = 0, 255
        return out
    if kind == "checker":
        return np.repeat((((x//8 + y//8) % 2)*255).astype(np.uint8)[..., None], 3, -1)
    if kind == "grey":
        return np.full((height, width, 3), 128, np.uint8)
    if kind == "sparse":
        terms = [(7, 7), (7, 0), (0, 7), (6, 7), (5, 5), (7, 3)]
        block = (y//8)*((width + 7)//8) + x//8
        value = np.zeros((height, width))
        for k, (v, u) in enumerate(terms):
            value += (block % len(terms) == k)*500.0*DCT[v][y % 8]*DCT[u][x % 8]
        return np.repeat(np.clip(np.rint(128 + value), 0, 255).astype(np.uint8)[..., None], 3, -1)
    raise ValueError(kind)


# seeds of the noise pictures of the coefficient tests: chosen on the CPU so that at qualities 50, 90 and 100 at most 1 % of the values in
# front of the rounding lie within 1e-3 of a tie (at quality 100 the DC, (0,4), (4,0) and (4,4) terms are multiples of 1/8: one in eight
# of them IS a tie, which alone is 0.8 % of a noise picture's terms)
NOISE_SEEDS = {(16, 16): 0, (48, 32): 2, (40, 24): 0, (17, 9): 0, (1040, 16): 24}


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    error = np.mean((a.astype(np.float64) - b.astype(np.float64))**2)
    return float("inf") if error == 0 else float(10*np.log10(255.0**2/error))
