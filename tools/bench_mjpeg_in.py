#!/usr/bin/env python3
"""One synthetic clip as rgb24 `.npy`, as `.y4m` and as Motion-JPEG `.avi` — with a restart interval per MCU row (what this package's
device encoder writes) and, when Pillow is there to write it, without restart markers (one interval per frame) — through the video
sequence (videosequence.py) at 1920x1080 and 3840x2160, render-only, all in one process: every configuration runs once untimed and
three times timed, the fastest run is reported with the spread, and the bytes a staged frame takes. Each `.avi` runs under both entropy
paths (csrc/jpeg_decode_kernels.hpp): a lane per restart interval (SHADERFLOW_JPEG_SYNC=0: the only path before the subsequence
path existed) and a lane per subsequence (SHADERFLOW_JPEG_SYNC=1) at several subsequence sizes (SHADERFLOW_JPEG_SYNC_BYTES), the
variants taking turns; one frame of each is decoded on both paths and compared first. Then, in runs of their own under
`rocprofv3 --kernel-trace --stats` (fresh child processes), both `.avi` again for the decode kernels' times. GPU box only.

    python tools/bench_mjpeg_in.py [--frames 60] [--out profiles/mjpeg_in_bench.txt] [--sizes 1920x1080 3840x2160] [--no-profile]
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
FPS, DISTINCT, QUALITY = 60.0, 8, 90


def pictures(width: int, height: int) -> np.ndarray:
    from shaderflow_amd import synth
    base = synth.background_image(width, height, seed=4)[..., :3].astype(np.uint8)
    return np.stack([np.roll(base, 8*k, axis=1) for k in range(DISTINCT)])


def write_avi(path: Path, streams: list, width: int, height: int) -> None:
    from shaderflow_amd.mjpeg import AviWriter
    fd = os.open(path, os.O_RDWR | os.O_CREAT | os.O_TRUNC)
    try:
        writer = AviWriter(fd, width, height, FPS)
        writer.begin()
        for stream in streams:
            writer.add(stream)
        writer.finish()
    finally:
        os.close(fd)


def device_streams(distinct: np.ndarray) -> list:
    """The pictures through this package's own encoder (a restart interval per MCU row)"""
    from shaderflow_amd.mjpegsource import AviReader
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    height, width = distinct.shape[1:3]

    class Show(ShaderScene):
        def build(self):
            self.video = ShaderVideo(scene=self, frames=distinct, fps=FPS)
            self.shader.fragment = "video"
    with tempfile.TemporaryDirectory(prefix="mjpeg_in_") as folder:
        Show().main(width=width, height=height, fps=FPS, time=len(distinct)/FPS, output=str(Path(folder)/"own.avi"), pixel_format="mjpeg", jpeg_quality=QUALITY)
        return list(AviReader(Path(folder)/"own.avi"))


def pillow_streams(distinct: np.ndarray):
    try:
        from PIL import Image
    except ImportError:
        return None
    out = []
    for picture in distinct:
        buffer = io.BytesIO()
        Image.fromarray(picture).save(buffer, "JPEG", quality=QUALITY, subsampling=2)
        out.append(buffer.getvalue())
    return out


def write_clips(folder: Path, width: int, height: int, frames: int) -> dict:
    distinct = pictures(width, height)
    order = [k % DISTINCT for k in range(frames)]
    np.save(folder/"clip.npy", distinct[order])
    with open(folder/"clip.y4m", "wb") as file:
        file.write(f"YUV4MPEG2 W{width} H{height} F{int(FPS)}:1 Ip C420jpeg\n".encode())
        planar = []
        for frame in distinct:
            r, g, b = (frame[..., k].astype(np.int32) for k in range(3))
            luma = (((66*r + 129*g + 25*b + 128) >> 8) + 16).astype(np.uint8)
            mean = [(c.reshape(height//2, 2, width//2, 2).sum(axis=(1, 3)) + 2) >> 2 for c in (r, g, b)]
            cb = (((-38*mean[0] - 74*mean[1] + 112*mean[2] + 128) >> 8) + 128).astype(np.uint8)
            cr = (((112*mean[0] - 94*mean[1] - 18*mean[2] + 128) >> 8) + 128).astype(np.uint8)
            planar.append(b"FRAME\n" + luma.tobytes() + cb.tobytes() + cr.tobytes())
        for k in order:
            file.write(planar[k])
    clips = {"npy": dict(path=folder/"clip.npy", fps=FPS), "y4m": dict(path=folder/"clip.y4m")}
    own = device_streams(distinct)
    write_avi(folder/"restart.avi", [own[k] for k in order], width, height)
    clips["avi, an interval per MCU row"] = dict(path=folder/"restart.avi")
    serial = pillow_streams(distinct)
    if serial is not None:
        write_avi(folder/"serial.avi", [serial[k] for k in order], width, height)
        clips["avi, no restart markers"] = dict(path=folder/"serial.avi")
    return clips


SYNC_SIZES = (64, 128, 256)
VARIANTS = {"a lane per interval": {"SHADERFLOW_JPEG_SYNC": "0"},
            **{f"subsequences of {size} bytes": {"SHADERFLOW_JPEG_SYNC": "1", "SHADERFLOW_JPEG_SYNC_BYTES": str(size)} for size in SYNC_SIZES}}


def run(source: dict, width: int, height: int, frames: int, switches: dict = {}):
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    os.environ["SHADERFLOW_VIDEO_SEQUENCE"] = "1"
    for name in ("SHADERFLOW_JPEG_SYNC", "SHADERFLOW_JPEG_SYNC_BYTES"):
        os.environ.pop(name, None)
    os.environ.update(switches)

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
    staged = scene.video.capacity if scene.video.format == "mjpeg" else width*height*3//(2 if scene.video.format == "i420" else 1)
    return took, staged


def same_on_both_paths(path: Path) -> str:
    """The clip's first frame through both entropy paths: its coefficients must not differ"""
    from shaderflow_amd.mjpegsource import AviReader, device_decode
    frame = next(iter(AviReader(path)))
    old = device_decode(frame)
    for size in SYNC_SIZES:
        new = device_decode(frame, sync=True, subsequence_bytes=size)
        if new["status"] or old["status"] or not np.array_equal(new["coefficients"], old["coefficients"]) or not np.array_equal(new["rgb"], old["rgb"]):
            raise RuntimeError(f"{path.name}: the subsequence path at {size} bytes differs from the lane-per-interval kernel (status {new['status']}, {old['status']})")
    return f"{new['sync']['subsequences']} subsequences of {SYNC_SIZES[-1]} bytes, {new['sync']['rounds_used']} rounds, fell back: {new['sync']['fell_back']}"


def profile_child(width: int, height: int, frames: int, clip: str) -> None:
    with tempfile.TemporaryDirectory(prefix="mjpeg_in_") as folder:
        clips = write_clips(Path(folder), width, height, frames)
        if clip in clips:
            run(clips[clip], width, height, frames, {"SHADERFLOW_JPEG_SYNC": "1"} if "no restart" in clip else {})


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=60)
    p.add_argument("--out", type=Path, default=ROOT/"profiles"/"mjpeg_in_bench.txt", help="the printed lines, appended")
    p.add_argument("--sizes", nargs="*", default=["1920x1080", "3840x2160"])
    p.add_argument("--no-profile", action="store_true")
    p.add_argument("--profile-child", default=None, help=argparse.SUPPRESS)
    p.add_argument("--profile-clip", default="avi, an interval per MCU row", help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.profile_child:
        width, height = map(int, args.profile_child.split("x"))
        return profile_child(width, height, args.frames, args.profile_clip)
    from shaderflow_amd import _native
    lines = []

    def say(line: str) -> None:
        lines.append(line)
        print(line, flush=True)
    say(f"# Motion-JPEG in (kernel sources {_native.source_fingerprint()}): {args.frames} frames at {FPS:g} fps through the video sequence, render-only, quality {QUALITY}, 4:2:0")
    for size in args.sizes:
        width, height = map(int, size.split("x"))
        with tempfile.TemporaryDirectory(prefix="mjpeg_in_") as folder:
            clips = write_clips(Path(folder), width, height, args.frames)
            for name, source in clips.items():
                variants = VARIANTS if name.startswith("avi") else {"": {}}
                if name.startswith("avi"):
                    say(f"{size:9s} {name:30s}: both paths give the same coefficients and pixels ({same_on_both_paths(source['path'])})")
                times = {variant: [] for variant in variants}
                for variant, switches in variants.items():
                    run(source, width, height, min(30, args.frames), switches)
                for _ in range(3):                                    # the variants take turns
                    for variant, switches in variants.items():
                        took, staged = run(source, width, height, args.frames, switches)
                        times[variant].append(took)
                for variant, runs in times.items():
                    label = f"{name}, {variant}" if variant else name
                    say(f"{size:9s} {label:58s}: {args.frames} frames in {min(runs)*1e3:8.1f} ms (of {', '.join(f'{t*1e3:.1f}' for t in runs)}) = {args.frames/min(runs):7.1f} frames/s, "
                        f"a slot holds {staged/1e6:6.2f} MB")
        if args.no_profile or not shutil.which("rocprofv3"):
            continue
        for clip in ("avi, an interval per MCU row", "avi, no restart markers"):
            with tempfile.TemporaryDirectory(prefix="mjpeg_in_prof_") as folder:
                done = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", folder, "-o", "run", "--output-format", "csv", "--",
                                       sys.executable, str(Path(__file__).resolve()), "--profile-child", size, "--profile-clip", clip, "--frames", str(args.frames)],
                                      cwd=ROOT, capture_output=True, text=True, timeout=600)
                if done.returncode != 0:
                    say(f"{size:9s} rocprofv3 run failed ({done.returncode}): {done.stderr.strip()[-300:]}")
                    continue
                for stats in Path(folder).rglob("*kernel_stats.csv"):
                    with open(stats, newline="") as file:
                        for row in csv.DictReader(file):
                            if "jpeg" in row["Name"] or "video" in row["Name"]:
                                say(f"{size:9s} rocprofv3 ({clip}{', subsequence path' if 'no restart' in clip else ''}) {row['Name'].split('(')[0][:40]:40s} calls {row['Calls']:>5s} "
                                    f"mean {float(row['AverageNs'])/1e3:9.1f} us")
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as file:
        file.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
