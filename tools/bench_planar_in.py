#!/usr/bin/env python3
"""Planar sources through the video sequence (videosequence.py) at 1920x1080 and 3840x2160, render-only, all in one process: 8-bit 4:2:0
through the I420 kernel (`k_video_frame`), then the same frames, 4:2:0 with interpolated chroma, 4:2:2 at 10 bits and 4:4:4 through the
general kernel (`k_video_planar`, csrc/video_kernels.hpp). The frames come from memory (`frames=`: eight distinct frames in turns, the
reader thread copies each into a pinned slot), so no disk is measured. Every case runs once untimed and three times timed, the cases
taking turns; the fastest run is reported with all three, and the bytes a staged frame takes.

A source at the I420 layout is the I420 kernel's (video.py): for the second case alone this tool switches that special case off
(`PlanarLayout.is_i420`), which nothing in the package does. The last line per size says whether the general kernel at that layout is
within the run-to-run spread of the I420 kernel — what a later change that retires the special case would want to know. GPU box only.

    python tools/bench_planar_in.py [--frames 60] [--out profiles/planar_in_bench.txt] [--sizes 1920x1080 3840x2160]
"""
import argparse
import itertools
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
FPS, DISTINCT = 60.0, 8

# name → (ShaderVideo's format and fields, whether the I420 special case stays on)
CASES = {
    "420 8 bit, k_video_frame (the I420 kernel)": (dict(format="i420"), True),
    "420 8 bit nearest, k_video_planar": (dict(format="yuv420p"), False),
    "420 8 bit linear, k_video_planar": (dict(format="yuv420p", chroma="linear"), True),
    "422 10 bit nearest, k_video_planar": (dict(format="yuv422p10le"), True),
    "444 8 bit, k_video_planar": (dict(format="yuv444p"), True),
}


def frames_of(fields: dict, width: int, height: int) -> list:
    from shaderflow_amd.planarsource import PlanarLayout
    layout = PlanarLayout.from_format(fields["format"])
    rng = np.random.default_rng(width + layout.depth)
    samples = layout.frame_bytes(width, height)//layout.sample_bytes
    return [rng.integers(0, 2**layout.depth, samples).astype(np.uint16 if layout.depth > 8 else np.uint8) for _ in range(DISTINCT)]


def run(fields: dict, special_case: bool, distinct: list, width: int, height: int, frames: int):
    from shaderflow_amd import planarsource
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    os.environ["SHADERFLOW_VIDEO_SEQUENCE"] = "1"
    kept = planarsource.PlanarLayout.is_i420
    if not special_case:
        planarsource.PlanarLayout.is_i420 = property(lambda self: False)
    try:
        class Video(ShaderScene):
            def build(self):
                self.video = ShaderVideo(scene=self, frames=itertools.cycle(distinct), width=width, height=height, fps=FPS, **fields)
                self.shader.fragment = "video"
        scene = Video()
        started = time.perf_counter()
        scene.main(width=width, height=height, fps=FPS, time=frames/FPS, freewheel=True)
        took = time.perf_counter() - started
    finally:
        planarsource.PlanarLayout.is_i420 = kept
    if scene.video_sequence is None or scene.video._read < frames - 2:
        raise RuntimeError(f"the scene did not take the video sequence, or showed only {scene.video._read} of {frames} source frames")
    expected = "i420" if (special_case and fields["format"] == "i420") else "planar"
    if scene.video.format != expected:
        raise RuntimeError(f"the source ran as {scene.video.format!r}, not {expected!r}")
    return took, distinct[0].nbytes


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=60)
    p.add_argument("--out", type=Path, default=ROOT/"profiles"/"planar_in_bench.txt", help="the printed lines, appended")
    p.add_argument("--sizes", nargs="*", default=["1920x1080", "3840x2160"])
    args = p.parse_args()
    from shaderflow_amd import _native
    lines = []

    def say(line: str) -> None:
        lines.append(line)
        print(line, flush=True)
    say(f"# planar sources in (kernel sources {_native.source_fingerprint()}): {args.frames} frames at {FPS:g} fps through the video sequence, render-only, frames from memory")
    for size in args.sizes:
        width, height = map(int, size.split("x"))
        clips = {name: frames_of(fields, width, height) for name, (fields, _) in CASES.items()}
        times = {name: [] for name in CASES}
        for name, (fields, special) in CASES.items():
            run(fields, special, clips[name], width, height, min(30, args.frames))
        staged = {}
        for _ in range(3):                                            # the cases take turns
            for name, (fields, special) in CASES.items():
                took, staged[name] = run(fields, special, clips[name], width, height, args.frames)
                times[name].append(took)
        for name, runs in times.items():
            say(f"{size:9s} {name:44s}: {args.frames} frames in {min(runs)*1e3:8.1f} ms (of {', '.join(f'{t*1e3:.1f}' for t in runs)}) = {args.frames/min(runs):7.1f} frames/s, "
                f"a slot holds {staged[name]/1e6:6.2f} MB")
        old, new = (times[name] for name in list(CASES)[:2])
        spread = max(old) - min(old)
        inside = abs(min(new) - min(old)) <= spread
        say(f"{size:9s} the general kernel at the I420 layout is {'within' if inside else 'OUTSIDE'} the I420 kernel's run-to-run spread: "
            f"fastest {min(new)*1e3:.1f} ms against {min(old)*1e3:.1f} ms, spread {spread*1e3:.1f} ms")
    args.out.parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as file:
        file.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
