"""
jpeg_streams.npz: small baseline JPEG streams for the Motion-JPEG source's tests, with the pixels libjpeg (through Pillow) decodes
from the same bytes, so that the tests need no Pillow. Run from the repository root: python tests/golden/make_golden_jpeg_streams.py

Per stream `<name>`: `<name>.stream` (uint8), `<name>.pillow` (height x width x 3 uint8, Pillow's own decode, grey repeated).
The shapes: 16x16 one MCU; 17x9 and 33x18 partial MCUs and odd chroma extents; 40x24 and 48x32; 16x1040 more than 64 restart intervals
(more than one wave of lanes); 1040x16 one long interval. Subsampling 4:4:4, 4:2:2, 4:2:0 and mode L; restart intervals none, one MCU
row and 3 MCUs; `optimize=True` (the file's own Huffman tables); one stream with its DHT segments stripped (Annex K tables implied).
Two streams are this project's own (tests/jpeg_ref.py `encode`): "extremes" (an 11-bit DC difference) and "sparse" (ZRL runs).
The noise seeds are chosen so that at most 1 % of the decoded samples lie within 1e-3 of a rounding tie (tests/test_host_mjpeg_in.py
asserts it).
"""
import io
import struct
import sys
from pathlib import Path

import numpy as np
from PIL import Image

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import jpeg_decode_ref as D  # noqa: E402
import jpeg_ref as J  # noqa: E402

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
# name: (width, height, picture, layout, restart: None | "row" | MCUs, optimize)
CASES = {
    "one_mcu_420": (16, 16, "noise", "420", None, False),
    "one_mcu_444": (16, 16, "gradient", "444", None, False),
    "partial_420": (17, 9, "noise", "420", "row", False),
    "partial_422": (17, 9, "noise", "422", 3, False),
    "partial_444": (17, 9, "gradient", "444", None, True),
    "odd_420": (33, 18, "noise", "420", 3, True),
    "odd_422": (33, 18, "noise", "422", "row", False),
    "odd_grey": (33, 18, "noise", "L", 3, False),
    "mid_420": (40, 24, "noise", "420", "row", False),
    "mid_444": (40, 24, "noise", "444", 3, False),
    "wide_422": (48, 32, "gradient", "422", None, True),
    "wide_420": (48, 32, "noise", "420", 3, False),
    "tall_420": (16, 1040, "noise", "420", "row", False),
    "tall_444": (16, 1040, "gradient", "444", 3, False),
    "long_420": (1040, 16, "noise", "420", "row", False),
    "long_grey": (1040, 16, "gradient", "L", None, False),
    "no_dht_420": (48, 32, "noise", "420", "row", False),
}


def strip_dht(stream: bytes) -> bytes:
    out, pos = bytearray(stream[:2]), 2
    while True:
        marker, length = stream[pos + 1], struct.unpack(">H", stream[pos + 2:pos + 4])[0]
        if marker != 0xc4:
            out += stream[pos:pos + 2 + length]
        pos += 2 + length
        if marker == 0xda:
            return bytes(out) + stream[pos:]


def pillow_stream(width, height, kind, layout, restart, optimize, seed):
    picture = J.picture(kind, width, height, seed)
    image = Image.fromarray(picture[..., 0] if layout == "L" else picture)
    options = dict(quality=90, optimize=optimize)
    if layout != "L":
        options["subsampling"] = SUBSAMPLING[layout]
    if restart == "row":
        options["restart_marker_rows"] = 1
    elif restart:
        options["restart_marker_blocks"] = restart
    buffer = io.BytesIO()
    image.save(buffer, "JPEG", **options)
    return buffer.getvalue()


def tie_share(stream: bytes) -> float:
    return float((D.tie_distance(D.decode(stream)["samples"]) < 1e-3).mean())


def main():
    out = {}
    for name, (width, height, kind, layout, restart, optimize) in CASES.items():
        for seed in range(64):
            stream = pillow_stream(width, height, kind, layout, restart, optimize, seed)
            if name.startswith("no_dht"):
                stream = strip_dht(stream)
            share = tie_share(stream)
            if share <= 0.01:
                break
            if kind != "noise":
                raise SystemExit(f"{name}: {share:.4f} of the samples within 1e-3 of a tie, and the picture has no seed to change")
        else:
            raise SystemExit(f"{name}: no seed below 64 keeps the ties under 1 %")
        pillow = np.asarray(Image.open(io.BytesIO(D.with_tables(stream))).convert("RGB"))
        info = D.decode(stream)
        print(f"{name}: {len(stream)} bytes, seed {seed}, ties {share*100:.3f} %, restart interval {info['restart_interval']}, sampling {info['sampling']}")
        out[f"{name}.stream"], out[f"{name}.pillow"] = np.frombuffer(stream, np.uint8), pillow
    for name, (kind, width, height, quality) in {"own_extremes": ("extremes", 48, 32, 100), "own_sparse": ("sparse", 40, 24, 90)}.items():
        for seed in range(64):
            stats = {}
            stream = J.encode(J.picture(kind, width, height, seed), quality, stats)
            share = tie_share(stream)
            if share <= 0.01:
                break
        else:
            raise SystemExit(f"{name}: no seed below 64 keeps the ties under 1 %")
        print(f"{name}: {len(stream)} bytes, seed {seed}, ties {share*100:.3f} %, {stats}")
        out[f"{name}.stream"] = np.frombuffer(stream, np.uint8)
        out[f"{name}.pillow"] = np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))
    np.savez_compressed(HERE/"jpeg_streams.npz", **out)
    print(f"{(HERE/'jpeg_streams.npz').stat().st_size} bytes")


if __name__ == "__main__":
    main()
