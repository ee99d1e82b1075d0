"""
staged_sha256.json: what `mjpegsource.stage` writes for every stream of jpeg_streams.npz, as the sha256 of the staged frame's bytes,
and the four Annex K Huffman tables as the device library states them. Run from the repository root:

    python tests/golden/make_golden_staged.py [--out tests/golden/staged_sha256.json]

"staged": stream name → sha256 of view[:total], the frame staged into a slot of `capacity_for(header, len(stream))` bytes. Recorded
BEFORE `stage` was rewritten over the `STAGED` record, so the test that reads it holds the rewrite to the bytes of the first version.
"annex_k": "<class><table>" → [BITS, HUFFVAL] as hex, read from the DHT segments of `sfx_jpeg_header` (csrc/jpeg_common.hpp's C
tables, as the encoder writes them into every frame). That half needs a device: without one the file's earlier "annex_k" is kept.
The committed "annex_k" was first written without a device, by a host-only program that printed jpeg_common.hpp's arrays; a run of this
script on a device writes the same tables from the encoder's header, or shows that they differ.
"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
from shaderflow_amd import mjpegsource as M  # noqa: E402


def staged() -> dict:
    data = np.load(HERE/"jpeg_streams.npz")
    out = {}
    for name in sorted(n[:-7] for n in data.files if n.endswith(".stream")):
        stream = data[name + ".stream"].tobytes()
        header = M.parse_header(stream)
        view = np.full(M.capacity_for(header, len(stream)), 0xaa, np.uint8)
        total = M.stage(stream, header, view)
        out[name] = hashlib.sha256(view[:total].tobytes()).hexdigest()
    return out


def annex_k() -> dict:
    """The Huffman tables of the encoder's constant header (any size and quality: they do not depend on either)"""
    from shaderflow_amd import _native as N
    encoder = N.JpegEncoder(N.default_context(), 16, 16, 90)
    try:
        tables = M.parse_header(encoder.header()).huffman
    finally:
        encoder.destroy()
    return {f"{kind}{table}": [bytes(bits).hex(), bytes(values).hex()] for (kind, table), (bits, values) in sorted(tables.items())}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", type=Path, default=HERE/"staged_sha256.json")
    args = parser.parse_args()
    earlier = json.loads(args.out.read_text()) if args.out.exists() else {}
    result = {"staged": staged()}
    try:
        result["annex_k"] = annex_k()
    except Exception as error:                                            # no library, or no device
        print(f"annex_k not read from the device ({error}): the file's earlier tables are kept")
        if "annex_k" in earlier:
            result["annex_k"] = earlier["annex_k"]
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(json.dumps(result, indent=1, sort_keys=True) + "\n")
    print(f"{args.out}: {len(result['staged'])} staged frames, annex_k {'there' if 'annex_k' in result else 'missing'}")


if __name__ == "__main__":
    main()
