#!/usr/bin/env python3
"""The 4K 2xSSAA Visualizer export as rgb24, mjpeg (quality 90) and png, measured in turns in one session: frames/s, mean bytes per
frame and the ratios between them, and — from `rocprofv3 --kernel-trace --stats` over a short png export in a process of its own — the
three PNG kernels' times. Writes profiles/png_bench.txt. GPU box only.

    python tools/bench_png.py [--frames 240] [--rounds 3] [--no-profile]

rgb24 goes to /dev/null. mjpeg and png go to an `.avi` file (memory-backed where /dev/shm exists): an AVI is seeked and truncated,
/dev/null will not do, and png has no other file container. AVI 1.0 holds 4 GiB, which bounds --frames for png at 4K.

`--opendml`: one export past 4 GiB alone — png with `opendml=True` (segments of 1 GiB), `--frames` of them (900 are about 4.55 GB) — then
the file read back: the frames `clips.AviClip` finds, the last one's offset, the RIFF chunks, and tests/odml_ref.py over the whole
file. The file is deleted afterwards; its lines are APPENDED to profiles/png_bench.txt. `--directory` says where it goes.
"""
import argparse
import csv
import os
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

W, H, SSAA, FPS = 3840, 2160, 2.0, 60.0
FORMATS = ("rgb24", "mjpeg", "png")


def visualizer():
    from examples.scenes import Visualizer, make
    from shaderflow_amd import synth
    return make(Visualizer, audio=(synth.sweep_clip(32.0, 44100), 44100), background=synth.background_image(1920, 1080, seed=0))


def export(pixel_format: str, frames: int, output) -> float:
    started = time.perf_counter()
    visualizer().main(width=W, height=H, ssaa=SSAA, fps=FPS, time=frames/FPS, output=output, pixel_format=pixel_format, jpeg_quality=90)
    return time.perf_counter() - started


def opendml_leg(frames: int, directory) -> list[str]:
    import mmap

    from shaderflow_amd import _native as N
    from shaderflow_amd import pngsource
    from tests import odml_ref
    with tempfile.TemporaryDirectory(dir=directory) as folder:
        free = shutil.disk_usage(folder).free
        need = frames*N.PngEncoder.capacity(W, H)//4                     # (a frame is about a fifth of its capacity)
        if free < need:
            return [f"opendml: no room for {frames} png frames in {folder}: {free} bytes free, about {need} needed: not run"]
        path = Path(folder)/"clip.avi"
        started = time.perf_counter()
        visualizer().main(width=W, height=H, ssaa=SSAA, fps=FPS, time=frames/FPS, output=path, pixel_format="png", opendml=True)
        took = time.perf_counter() - started
        size = path.stat().st_size
        clip = pngsource.AviReader(path)
        count, last, largest = len(clip), clip.index[-1], clip.largest
        clip.close()
        with open(path, "rb") as file, mmap.mmap(file.fileno(), 0, access=mmap.ACCESS_READ) as data:
            avi = odml_ref.parse(data)
            walked = avi["walk"][b"00dc"]
            spans = odml_ref.spans(avi)
        path.unlink()
    return [f"opendml: png to an .avi file in {folder.rsplit('/', 1)[0]}, {frames} frames, segments of 1 GiB, kernel sources {N.source_fingerprint()}",
            f"  {size} bytes ({size/2**32:.3f} x 4 GiB) in {took:.2f} s = {frames/took:.0f} frames/s (one run), {size/frames:.0f} bytes per frame, the largest {largest}",
            f"  AviClip: {count} frames, the last at byte {last[0]} ({last[1]} bytes){', past 2^32' if last[0] > 1 << 32 else ''}",
            f"  odml_ref: valid; {len(spans)} RIFF chunks of {', '.join(str(span) for span in spans)} bytes; {len(walked)} frames by walk and by index, "
            f"the same places as AviClip's: {walked == clip.index}"]


def kernel_times(frames: int) -> list[str]:
    """rocprofv3's per-kernel statistics of a short png export in a fresh process: the lines of the PNG kernels"""
    rocprof = shutil.which("rocprofv3")
    if rocprof is None:
        return ["rocprofv3 not found: no kernel times"]
    with tempfile.TemporaryDirectory() as directory:
        command = [rocprof, "--kernel-trace", "--stats", "-d", directory, "-o", "png", "--output-format", "csv", "--",
                   sys.executable, str(Path(__file__).resolve()), "--child", "--frames", str(frames)]
        done = subprocess.run(command, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            return [f"rocprofv3 run failed ({done.returncode}): {done.stderr.strip()[-300:]}"]
        lines = []
        for path in Path(directory).rglob("*kernel_stats.csv"):
            with open(path, newline="") as file:
                for row in csv.DictReader(file):
                    if "k_png_" in row.get("Name", ""):
                        name = row["Name"].split("(")[0].split("::")[-1]
                        lines.append(f"  {name:22s} {int(row['Calls']):5d} calls, {float(row['TotalDurationNs'])/1e3/frames:8.1f} us per frame, "
                                     f"{float(row['AverageNs'])/1e3:9.1f} us per call, {float(row['Percentage']):5.2f} % of the kernel time")
        return lines or ["no k_png_* rows in rocprofv3's kernel statistics"]


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--frames", type=int, default=240)
    parser.add_argument("--rounds", type=int, default=3, help="turns of rgb24, mjpeg, png; the first is not measured")
    parser.add_argument("--child", action="store_true", help="(internal) one png export, nothing else")
    parser.add_argument("--no-profile", action="store_true")
    parser.add_argument("--opendml", action="store_true", help="one png export past 4 GiB with opendml=True, read back; appended to profiles/png_bench.txt")
    parser.add_argument("--directory", default=None, help="where --opendml's file goes (the temporary directory by default)")
    args = parser.parse_args()
    if args.opendml:
        lines = opendml_leg(args.frames, args.directory)
        with open(ROOT/"profiles"/"png_bench.txt", "a") as file:
            file.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    shm = "/dev/shm" if os.path.isdir("/dev/shm") else None
    if args.child:
        with tempfile.TemporaryDirectory(dir=shm) as directory:
            export("png", args.frames, Path(directory)/"clip.avi")
        return
    from shaderflow_amd import _native as N
    rates: dict = {name: [] for name in FORMATS}
    sizes: dict = {"rgb24": W*H*3}
    with tempfile.TemporaryDirectory(dir=shm) as directory:
        for turn in range(args.rounds):
            for name in FORMATS:
                path = Path(directory)/"clip.avi"
                took = export(name, args.frames, "/dev/null" if name == "rgb24" else path)
                if name != "rgb24":
                    sizes[name] = path.stat().st_size/args.frames
                    path.unlink()
                if turn:
                    rates[name].append(args.frames/took)
                print(f"turn {turn} {name:6s}: {args.frames/took:7.0f} frames/s", flush=True)
    mean = (lambda values: sum(values)/max(1, len(values)))
    lines = [f"4K 2xSSAA Visualizer export, {args.frames} frames, rgb24 to /dev/null, mjpeg q90 and png to an .avi file in {shm or 'the temporary directory'}; "
             f"{args.rounds} turns of the three, the first not measured; kernel sources {N.source_fingerprint()}",
             f"capacity of a png sink frame: {N.PngEncoder.capacity(W, H)} bytes"]
    for name in FORMATS:
        lines.append(f"{name:6s}: {', '.join(f'{r:.0f}' for r in rates[name])} frames/s (mean {mean(rates[name]):.0f}), {sizes[name]:10.0f} bytes per frame"
                     + (f" ({sizes['rgb24']/sizes[name]:.2f} x smaller than rgb24)" if name != "rgb24" else ""))
    lines.append(f"png / mjpeg: {sizes['png']/sizes['mjpeg']:.2f} x the bytes, {mean(rates['png'])/max(1e-9, mean(rates['mjpeg'])):.2f} x the frames/s; "
                 f"png / rgb24: {mean(rates['png'])/max(1e-9, mean(rates['rgb24'])):.2f} x the frames/s")
    if not args.no_profile:
        lines.append("rocprofv3 --kernel-trace --stats, png, 36 frames, a process of its own:")
        lines += kernel_times(36)
    (ROOT/"profiles").mkdir(exist_ok=True)
    (ROOT/"profiles"/"png_bench.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
