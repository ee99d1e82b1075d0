#!/usr/bin/env python3
"""PNG in: the Visualizer example exported by this package (`pixel_format="png"`: an IDAT chunk per stripe of 8 rows) read back through
the video sequence (videosequence.py), render-only, at 1920x1080 and 3840x2160 — under SHADERFLOW_PNG_SEGMENTS=1 (a wave per IDAT
chunk) and =0 (the serial path: one wave inflates the frame) — beside the same frames written by Pillow at its default level (one
deflate stream: the serial path), and the same clip as `.y4m` and `.npy`. Every configuration runs once untimed and `--runs` times
timed; the fastest run is reported with the spread. The serial path is slow by construction, so its runs show `--serial-frames` frames
only. Then, in a run of its own under `rocprofv3 --kernel-trace --stats` (a fresh child process), the own clip again for the PNG
kernels' times. GPU box only.

    python tools/bench_png_in.py [--frames 60] [--serial-frames 6] [--runs 3] [--out profiles/png_in_bench.txt] [--sizes 1920x1080 3840x2160] [--no-profile]
"""
import argparse
import csv
import io
import os
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
FPS, DISTINCT = 60.0, 8


def write_avi(path: Path, streams: list, width: int, height: int) -> None:
    from shaderflow_amd.mjpeg import AviWriter
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        writer = AviWriter(fd, width, height, FPS, fourcc=b"MPNG")
        writer.begin()
        for stream in streams:
            writer.add(stream)
        writer.finish()
    finally:
        os.close(fd)


def visualizer_streams(folder: Path, width: int, height: int) -> list:
    """DISTINCT frames of the Visualizer example through this package's own PNG encoder"""
    from examples.scenes import Visualizer, make
    from shaderflow_amd import synth
    from shaderflow_amd.pngsource import AviReader
    scene = make(Visualizer, audio=(synth.sweep_clip(1.0, 44100), 44100), background=synth.background_image(480, 270, seed=2))
    scene.main(width=width, height=height, fps=FPS, time=DISTINCT/FPS, output=str(folder/"own8.avi"), pixel_format="png")
    return list(AviReader(folder/"own8.avi"))


def write_clips(folder: Path, width: int, height: int, frames: int) -> dict:
    from PIL import Image
    own = visualizer_streams(folder, width, height)
    distinct = np.stack([np.asarray(Image.open(io.BytesIO(stream)).convert("RGB")) for stream in own])
    order = [k % DISTINCT for k in range(frames)]
    np.save(folder/"clip.npy", distinct[order])
    with open(folder/"clip.y4m", "wb") as file:
        file.write(f"YUV4MPEG2 W{width} H{height} F{int(FPS)}:1 Ip C420jpeg\n".encode())
        for k in order:
            r, g, b = (distinct[k][..., c].astype(np.int32) for c in range(3))
            luma = (((66*r + 129*g + 25*b + 128) >> 8) + 16).astype(np.uint8)
            mean = [(c.reshape(height//2, 2, width//2, 2).sum(axis=(1, 3)) + 2) >> 2 for c in (r, g, b)]
            cb = (((-38*mean[0] - 74*mean[1] + 112*mean[2] + 128) >> 8) + 128).astype(np.uint8)
            cr = (((112*mean[0] - 94*mean[1] - 18*mean[2] + 128) >> 8) + 128).astype(np.uint8)
            file.write(b"FRAME\n" + luma.tobytes() + cb.tobytes() + cr.tobytes())
    pillow = []
    for picture in distinct:
        buffer = io.BytesIO()
        Image.fromarray(picture).save(buffer, "PNG")
        pillow.append(buffer.getvalue())
    write_avi(folder/"own.avi", [own[k] for k in order], width, height)
    write_avi(folder/"pillow.avi", [pillow[k] for k in order], width, height)
    return {"npy": dict(path=folder/"clip.npy", fps=FPS), "y4m": dict(path=folder/"clip.y4m"),
            "avi, own export (an IDAT per stripe)": dict(path=folder/"own.avi"), "avi, Pillow (one stream)": dict(path=folder/"pillow.avi")}


def run(source: dict, width: int, height: int, frames: int, switches=()):
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    os.environ["SHADERFLOW_VIDEO_SEQUENCE"] = "1"
    os.environ.pop("SHADERFLOW_PNG_SEGMENTS", None)
    os.environ.update(dict(switches))

    class Video(ShaderScene):
        def build(self):
            self.video = ShaderVideo(scene=self, **source)
            self.shader.fragment = "video"
    scene = Video()
    started = time.perf_counter()
    scene.main(width=width, height=height, fps=FPS, time=frames/FPS, freewheel=True)
    took = time.perf_counter() - started
    if scene.video_sequence is None or scene.video._read < frames - 2:
        raise RuntimeError(f"the scene did not take the video sequence, or showed only {scene.video._read} of {frames} source frames")
    staged = scene.video.capacity if scene.video.format == "png" else width*height*3//(2 if scene.video.format == "i420" else 1)
    return took, staged


def same_on_both_paths(path: Path) -> str:
    from shaderflow_amd.pngsource import AviReader, device_decode
    frame = next(iter(AviReader(path)))
    serial, parallel = device_decode(frame, segments=False), device_decode(frame, segments=True)
    if serial["status"] or parallel["status"] or not np.array_equal(serial["rgb"], parallel["rgb"]) or not np.array_equal(serial["filtered"], parallel["filtered"]):
        raise RuntimeError(f"{path.name}: the segment path differs from the serial path (status {parallel['status']}, {serial['status']})")
    from PIL import Image
    if not np.array_equal(parallel["rgb"], np.asarray(Image.open(io.BytesIO(frame)).convert("RGB"))):
        raise RuntimeError(f"{path.name}: the device's pixels are not Pillow's")
    return f"{parallel['info']['segments']} segments, parallel: {parallel['info']['parallel']}, fell back: {parallel['info']['fell_back']}, {len(frame)/1e6:.2f} MB a frame"


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=60)
    p.add_argument("--serial-frames", type=int, default=6)
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--out", type=Path, default=ROOT/"profiles"/"png_in_bench.txt", help="the printed lines, appended")
    p.add_argument("--sizes", nargs="*", default=["1920x1080", "3840x2160"])
    p.add_argument("--no-profile", action="store_true")
    p.add_argument("--profile-child", default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.profile_child:
        width, height = map(int, args.profile_child.split("x"))
        with tempfile.TemporaryDirectory(prefix="png_in_") as folder:
            run(write_clips(Path(folder), width, height, args.frames)["avi, own export (an IDAT per stripe)"], width, height, args.frames)
        return
    from shaderflow_amd import _native
    args.out.parent.mkdir(parents=True, exist_ok=True)

    def say(line: str) -> None:                                       # (appended line by line: a run that is cut short keeps what it measured)
        print(line, flush=True)
        with open(args.out, "a") as file:
            file.write(line + "\n")
    say(f"# PNG in (kernel sources {_native.source_fingerprint()}): frames at {FPS:g} fps through the video sequence, render-only; the Visualizer example's frames")
    for size in args.sizes:
        width, height = map(int, size.split("x"))
        with tempfile.TemporaryDirectory(prefix="png_in_") as folder:
            clips = write_clips(Path(folder), width, height, args.frames)
            for name, source in clips.items():
                variants = {"": {}}
                if name.startswith("avi, own"):
                    say(f"{size:9s} {name:38s}: both paths give the same stream and Pillow's pixels ({same_on_both_paths(source['path'])})")
                    variants = {"segment path": {"SHADERFLOW_PNG_SEGMENTS": "1"}, "serial path": {"SHADERFLOW_PNG_SEGMENTS": "0"}}
                elif name.startswith("avi"):
                    variants = {"serial path": {}}
                for variant, switches in variants.items():
                    frames = args.serial_frames if variant == "serial path" else args.frames
                    run(source, width, height, min(frames, 8), switches)
                    runs = [run(source, width, height, frames, switches) for _ in range(1 if variant == "serial path" else args.runs)]
                    best = min(took for took, _ in runs)
                    label = f"{name}, {variant}" if variant else name
                    say(f"{size:9s} {label:52s}: {frames} frames in {best*1e3:9.1f} ms (of {', '.join(f'{t*1e3:.1f}' for t, _ in runs)}) = {frames/best:7.1f} frames/s, "
                        f"a slot holds {runs[0][1]/1e6:6.2f} MB")
        if args.no_profile or not shutil.which("rocprofv3"):
            continue
        with tempfile.TemporaryDirectory(prefix="png_in_prof_") as folder:
            done = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", folder, "-o", "run", "--output-format", "csv", "--",
                                   sys.executable, str(Path(__file__).resolve()), "--profile-child", size, "--frames", str(min(args.frames, 16))],
                                  cwd=ROOT, capture_output=True, text=True, timeout=600)
            if done.returncode != 0:
                say(f"{size:9s} rocprofv3 run failed ({done.returncode}): {done.stderr.strip()[-300:]}")
                continue
            for stats in Path(folder).rglob("*kernel_stats.csv"):
                with open(stats, newline="") as file:
                    for row in csv.DictReader(file):
                        if "k_png_inflate" in row["Name"] or "k_png_adler" in row["Name"] or "k_png_check" in row["Name"] or "k_png_unfilter" in row["Name"]:
                            say(f"{size:9s} rocprofv3 (own export, segment path) {row['Name'].split('(')[0][:40]:40s} calls {row['Calls']:>5s} mean {float(row['AverageNs'])/1e3:9.1f} us")


if __name__ == "__main__":
    main()
