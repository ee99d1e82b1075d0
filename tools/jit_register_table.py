#!/usr/bin/env python3
"""VGPR / SGPR / scratch / LDS of every kernel of the translated fragments the project ships (tests/golden/jit/*.glsl and
examples/scenes.py::Bloom, with and without its LDS tile), read from the notes of freshly cross-compiled gfx950 code objects.
No GPU needed. Run it before and after a change to csrc/glsl.hpp or csrc/jit_runtime.hpp: a header change that is meant to leave
the existing fragments alone leaves this table alone (DESIGN.md §5 keeps the last one).
usage: tools/jit_register_table.py [output.txt]"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from shaderflow_amd import glsl2hip as G      # noqa: E402

LLVM = Path(G.HIPCC).resolve().parent.parent/"lib"/"llvm"/"bin"


def bloom_fragment() -> str:
    text = (ROOT/"examples"/"scenes.py").read_text()
    return re.search(r'class Bloom\(.*?FRAGMENT = """(.*?)"""', text, re.S).group(1)


def units():
    for path in sorted((ROOT/"tests"/"golden"/"jit").glob("*.glsl")):
        yield path.stem, path.read_text(), "1"
    yield "Bloom.tiled", bloom_fragment(), "1"
    yield "Bloom.untiled", bloom_fragment(), "0"


def stats(name: str, cpp: str, directory: Path) -> list[str]:
    unit, code = directory/f"{name}.hip", directory/f"{name}.hsaco"
    unit.write_text(cpp)
    done = subprocess.run([G.HIPCC, *G.FLAGS, f"-I{G.CSRC}", "--genco", str(unit), "-o", str(code)], capture_output=True, text=True)
    if done.returncode:
        return [f"{name}: hipcc failed\n{done.stderr[-2000:]}"]
    elf = code
    if code.read_bytes()[:4] != b"\x7fELF":
        elf = directory/f"{name}.o"
        subprocess.run([LLVM/"clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={code}", f"--output={elf}"],
                       check=True, capture_output=True)
    notes = subprocess.run([LLVM/"llvm-readelf", "--notes", str(elf)], capture_output=True, text=True).stdout
    rows = []
    for block in notes.split("- .agpr_count")[1:]:
        kernel = re.search(r"\.name:\s+(\S+)", block)
        if not kernel:
            continue
        get = lambda key: (re.search(rf"\.{key}:\s+(\d+)", block) or [None, "?"])[1]
        rows.append(f"{name:14s} {kernel.group(1):22s} vgpr {get('vgpr_count'):>4s} sgpr {get('sgpr_count'):>4s} scratch {get('private_segment_fixed_size'):>5s} "
                    f"lds {get('group_segment_fixed_size'):>6s}")
    return sorted(rows)


def main():
    jobs = []
    for name, text, tile in units():
        os.environ["SHADERFLOW_JIT_TILE"] = tile
        jobs.append((name, G.translate(text, [("sampler2D", "background")]).cpp))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(8) as pool:
        table = [row for rows in pool.map(lambda job: stats(*job, Path(tmp)), jobs) for row in rows]
    text = "\n".join(table) + "\n"
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(text)
    print(text, end="")


if __name__ == "__main__":
    main()
