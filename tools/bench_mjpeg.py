#!/usr/bin/env python3
"""The 4K 2xSSAA Visualizer export to /dev/null, 1 800 frames, as rgb24, yuv420p and mjpeg (quality 90 and 75): frames/s, mean bytes per
frame, and — from `rocprofv3 --kernel-trace --stats` over a short mjpeg export in a process of its own — the three JPEG kernels' times.
Writes profiles/mjpeg_bench.txt. GPU box only.

    python tools/bench_mjpeg.py [--frames 1800] [--no-profile]

`--sound-track`: the sound-track leg alone — the same export at quality 90 to an `.avi` file (memory-backed where /dev/shm exists: an
AVI is seeked and truncated, /dev/null will not do), with and without `sound_track=True`, taking turns, three runs each after one
unmeasured run of both. Its lines are APPENDED to profiles/mjpeg_bench.txt.

`--opendml [BYTES]`: the OpenDML leg alone, measured the same way — the `.avi` export at quality 90 with and without `opendml=BYTES`
(64 MiB by default, so that a 900-frame export of about half a gigabyte is cut several times: the default segment of 1 GiB would never
be reached, and the writer thread's comparison runs per frame either way). Its lines are APPENDED to profiles/mjpeg_bench.txt.
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


def visualizer():
    from examples.scenes import Visualizer, make
    from shaderflow_amd import synth
    return make(Visualizer, audio=(synth.sweep_clip(32.0, 44100), 44100), background=synth.background_image(1920, 1080, seed=0))


def export(pixel_format: str, quality: int, frames: int, output, **options) -> tuple[float, object]:
    started = time.perf_counter()
    result = visualizer().main(width=W, height=H, ssaa=SSAA, fps=FPS, time=frames/FPS, output=output, pixel_format=pixel_format, jpeg_quality=quality, **options)
    return time.perf_counter() - started, result


def sound_track_leg(frames: int) -> list[str]:
    """frames/s of the `.avi` export with and without the track, run in turns in this process"""
    from shaderflow_amd import _native as N
    rates: dict = {False: [], True: []}
    sizes: dict = {}
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as directory:
        for run in range(4):                                            # the first of each is not measured
            for track in (False, True):
                path = Path(directory)/"clip.avi"
                took, _ = export("mjpeg", 90, frames, path, sound_track=track)
                sizes[track] = path.stat().st_size
                path.unlink()
                if run:
                    rates[track].append(frames/took)
                    print(f"run {run} {'with' if track else 'without'} the track: {frames/took:7.0f} frames/s", flush=True)
    without, with_track = rates[False], rates[True]
    spread = max(without) - min(without)
    mean = (lambda values: sum(values)/len(values))
    lines = [f"sound track: mjpeg q90 to an .avi file in {'/dev/shm' if os.path.isdir('/dev/shm') else 'the temporary directory'}, {frames} frames, "
             f"three runs each in turns after one unmeasured run of both, kernel sources {N.source_fingerprint()}",
             f"  without the track: {', '.join(f'{r:.0f}' for r in without)} frames/s (mean {mean(without):.0f}, spread {spread:.0f}), {sizes[False]} bytes",
             f"  with the track   : {', '.join(f'{r:.0f}' for r in with_track)} frames/s (mean {mean(with_track):.0f}), {sizes[True]} bytes "
             f"({(sizes[True] - sizes[False])/frames:.0f} more per frame)",
             f"  mean with - mean without = {mean(with_track) - mean(without):+.0f} frames/s: "
             + ("within" if mean(without) - mean(with_track) <= spread else "BELOW the no-track runs by more than") + " the spread among the no-track runs"]
    return lines


def opendml_leg(frames: int, budget: int) -> list[str]:
    """frames/s of the `.avi` export with and without `opendml=budget`, run in turns in this process"""
    from shaderflow_amd import _native as N
    from shaderflow_amd.clips import AviClip
    from shaderflow_amd import mjpegsource
    rates: dict = {False: [], True: []}
    sizes: dict = {}
    counts: dict = {}
    where = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=where) as directory:
        for run in range(4):                                            # the first of each is not measured
            for segmented in (False, True):
                path = Path(directory)/"clip.avi"
                took, _ = export("mjpeg", 90, frames, path, opendml=budget if segmented else None)
                sizes[segmented] = path.stat().st_size
                if run == 3:
                    clip = AviClip(path, (mjpegsource,))
                    counts[segmented] = (len(clip), path.read_bytes().count(b"AVIX"))
                    clip.close()
                path.unlink()
                if run:
                    rates[segmented].append(frames/took)
                    print(f"run {run} {'with' if segmented else 'without'} opendml: {frames/took:7.0f} frames/s", flush=True)
    without, with_segments = rates[False], rates[True]
    spread = max(without) - min(without)
    mean = (lambda values: sum(values)/len(values))
    lines = [f"opendml: mjpeg q90 to an .avi file in {where or 'the temporary directory'}, {frames} frames, segments of {budget} bytes, "
             f"three runs each in turns after one unmeasured run of both, kernel sources {N.source_fingerprint()}",
             f"  without opendml: {', '.join(f'{r:.0f}' for r in without)} frames/s (mean {mean(without):.0f}, spread {spread:.0f}), {sizes[False]} bytes, "
             f"{counts[False][0]} frames read back",
             f"  with opendml   : {', '.join(f'{r:.0f}' for r in with_segments)} frames/s (mean {mean(with_segments):.0f}), {sizes[True]} bytes, "
             f"{counts[True][0]} frames read back from {counts[True][1] + 1} RIFF chunks",
             f"  mean with - mean without = {mean(with_segments) - mean(without):+.0f} frames/s: "
             + ("within" if mean(without) - mean(with_segments) <= spread else "BELOW the AVI 1.0 runs by more than") + " the spread among the runs without opendml"]
    return lines


def kernel_times(quality: int, frames: int) -> list[str]:
    """rocprofv3's per-kernel statistics of a short mjpeg export in a fresh process: the lines of the JPEG kernels"""
    rocprof = shutil.which("rocprofv3")
    if rocprof is None:
        return ["rocprofv3 not found: no kernel times"]
    with tempfile.TemporaryDirectory() as directory:
        command = [rocprof, "--kernel-trace", "--stats", "-d", directory, "-o", "mjpeg", "--output-format", "csv", "--",
                   sys.executable, str(Path(__file__).resolve()), "--child", str(quality), "--frames", str(frames)]
        done = subprocess.run(command, cwd=ROOT, capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            return [f"rocprofv3 run failed ({done.returncode}): {done.stderr.strip()[-300:]}"]
        lines = []
        for path in Path(directory).rglob("*kernel_stats.csv"):
            with open(path, newline="") as file:
                for row in csv.DictReader(file):
                    if "k_jpeg_" in row.get("Name", ""):
                        name = row["Name"].split("(")[0].split("::")[-1]
                        lines.append(f"  {name:22s} {int(row['Calls']):5d} calls, {float(row['TotalDurationNs'])/1e3/frames:8.1f} us per frame, "
                                     f"{float(row['AverageNs'])/1e3:9.1f} us per call, {float(row['Percentage']):5.2f} % of the kernel time")
        return lines or ["no k_jpeg_* rows in rocprofv3's kernel statistics"]


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--frames", type=int, default=1800)
    parser.add_argument("--child", type=int, default=None, help="(internal) one mjpeg export at this quality, nothing else")
    parser.add_argument("--no-profile", action="store_true")
    parser.add_argument("--sound-track", action="store_true", help="the sound-track leg alone, appended to profiles/mjpeg_bench.txt")
    parser.add_argument("--opendml", type=int, nargs="?", const=64 << 20, default=None, metavar="BYTES",
                        help="the OpenDML leg alone (segments of BYTES, 64 MiB by default), appended to profiles/mjpeg_bench.txt")
    args = parser.parse_args()
    if args.opendml is not None:
        lines = opendml_leg(args.frames, args.opendml)
        with open(ROOT/"profiles"/"mjpeg_bench.txt", "a") as file:
            file.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    if args.sound_track:
        lines = sound_track_leg(args.frames)
        with open(ROOT/"profiles"/"mjpeg_bench.txt", "a") as file:
            file.write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return
    if args.child is not None:
        with tempfile.TemporaryDirectory() as directory:
            os.symlink("/dev/null", Path(directory)/"null.mjpeg")
            export("mjpeg", args.child, args.frames, Path(directory)/"null.mjpeg")
        return
    from shaderflow_amd import _native as N
    lines = [f"4K 2xSSAA Visualizer export to /dev/null, {args.frames} frames (second of two runs each), kernel sources {N.source_fingerprint()}",
             f"rgb24 frame: {W*H*3} bytes; yuv420p: {W*H*3//2}"]
    with tempfile.TemporaryDirectory() as directory:
        null = Path(directory)/"null.mjpeg"
        os.symlink("/dev/null", null)
        for pixel_format, quality in (("rgb24", 0), ("yuv420p", 0), ("mjpeg", 90), ("mjpeg", 75)):
            for attempt in range(2):
                took, _ = export(pixel_format, quality or 90, args.frames, null if pixel_format == "mjpeg" else "/dev/null")
            line = f"{pixel_format:8s}{f' q{quality}' if quality else '    '}: {args.frames} frames in {took:7.3f} s = {args.frames/took:7.0f} frames/s"
            if pixel_format == "mjpeg":
                _, stream = export(pixel_format, quality, 60, "pipe")
                line += f", mean {len(stream)/60:9.0f} bytes per frame over the first 60 ({W*H*3/(len(stream)/60):.1f} x smaller than rgb24)"
            lines.append(line)
            print(line, flush=True)
    if not args.no_profile:
        for quality in (90, 75):
            lines.append(f"rocprofv3 --kernel-trace --stats, mjpeg q{quality}, 120 frames, a process of its own:")
            lines += kernel_times(quality, 120)
    (ROOT/"profiles").mkdir(exist_ok=True)
    (ROOT/"profiles"/"mjpeg_bench.txt").write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
