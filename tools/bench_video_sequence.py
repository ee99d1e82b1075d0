#!/usr/bin/env python3
"""Video (examples/scenes.py: the stock video fragment over a ShaderVideo) at 1920x1080 with a 1920x1080 synthetic clip (shaderflow_amd.synth)
whose frame rate is the scene's, so that every scene frame lands a source frame: the frame loop (SHADERFLOW_VIDEO_SEQUENCE=0: scene.next
per frame, ShaderVideo.update() with its flipped host copy and synchronous upload) against the VideoSequence (videosequence.py), for the
sources rgb24 `.npy`, raw `.rgb` and `.y4m`, render-only (freewheel, no sink) and rgb24 to /dev/null, at 1x and 2x SSAA, all in one
process. Every configuration runs once untimed (the contexts, the caches, the clip in the page cache) and then twice timed; the faster
timed run is reported. GPU box only.

    python tools/bench_video_sequence.py [--frames 120] [--out profiles/video_sequence_bench.txt] [--root CHECKOUT]

`--root`: measure the package of another checkout (the parent commit's frame loop, for the record in DESIGN §2e). A checkout without the
sequence runs its frame loop only, and a source it cannot read is reported as such.
"""
import argparse
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

WIDTH, HEIGHT, FPS = 1920, 1080, 60.0


def write_clips(folder: Path, frames: int) -> dict:
    """The same synthetic pictures as rgb24 (.npy, .rgb) and, converted once on the host with the yuv420p output's BT.601 integers, as .y4m"""
    from shaderflow_amd import synth
    base = synth.background_image(WIDTH, HEIGHT, seed=4)[..., :3].astype(np.uint8)
    clip = np.empty((frames, HEIGHT, WIDTH, 3), np.uint8)
    for k in range(frames):
        clip[k] = np.roll(base, 8*k, axis=1)                           # a picture that moves, so that a held frame would show
    np.save(folder/"clip.npy", clip)
    (folder/"clip.rgb").write_bytes(clip.tobytes())
    with open(folder/"clip.y4m", "wb") as file:
        file.write(f"YUV4MPEG2 W{WIDTH} H{HEIGHT} F{int(FPS)}:1 Ip C420jpeg\n".encode())
        for frame in clip:
            r, g, b = (frame[..., k].astype(np.int32) for k in range(3))
            luma = (((66*r + 129*g + 25*b + 128) >> 8) + 16).astype(np.uint8)
            mean = [(c.reshape(HEIGHT//2, 2, WIDTH//2, 2).sum(axis=(1, 3)) + 2) >> 2 for c in (r, g, b)]
            cb = (((-38*mean[0] - 74*mean[1] + 112*mean[2] + 128) >> 8) + 128).astype(np.uint8)
            cr = (((112*mean[0] - 94*mean[1] - 18*mean[2] + 128) >> 8) + 128).astype(np.uint8)
            file.write(b"FRAME\n" + luma.tobytes() + cb.tobytes() + cr.tobytes())
    return {"npy": dict(path=folder/"clip.npy", fps=FPS), "rgb": dict(path=folder/"clip.rgb", width=WIDTH, height=HEIGHT, fps=FPS),
            "y4m": dict(path=folder/"clip.y4m")}


def run(source: dict, frames: int, ssaa: float, sequence: bool, sink: str) -> float:
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    os.environ["SHADERFLOW_VIDEO_SEQUENCE"] = "1" if sequence else "0"

    class Video(ShaderScene):
        def build(self):
            self.video = ShaderVideo(scene=self, **source)
            self.shader.fragment = "video"
    scene = Video()
    started = time.perf_counter()
    if sink == "render":
        scene.main(width=WIDTH, height=HEIGHT, ssaa=ssaa, fps=FPS, time=frames/FPS, freewheel=True)
    else:
        scene.main(width=WIDTH, height=HEIGHT, ssaa=ssaa, fps=FPS, time=frames/FPS, output="/dev/null")
    took = time.perf_counter() - started
    if (getattr(scene, "video_sequence", None) is not None) != sequence:
        raise RuntimeError(f"expected the {'video sequence' if sequence else 'frame loop'}, the scene took the other path")
    if scene.video._read < frames - 2:
        raise RuntimeError(f"only {scene.video._read} of {frames} source frames were shown")
    return took


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=120)
    p.add_argument("--out", type=Path, default=None, help="the printed lines, appended")
    p.add_argument("--root", type=Path, default=Path(__file__).resolve().parent.parent, help="the checkout whose package is measured")
    p.add_argument("--ssaa", type=float, nargs="*", default=[1.0, 2.0])
    p.add_argument("--sources", nargs="*", default=["npy", "rgb", "y4m"])
    args = p.parse_args()
    sys.path.insert(0, str(args.root.resolve()))
    import shaderflow_amd
    from shaderflow_amd import _native
    has_sequence = (Path(shaderflow_amd.__file__).parent/"videosequence.py").exists()
    lines = []

    def say(line: str) -> None:
        lines.append(line)
        print(line, flush=True)
    say(f"# checkout {'with' if has_sequence else 'without'} the video sequence (kernel sources {_native.source_fingerprint()}), {args.frames} frames of {WIDTH}x{HEIGHT} at {FPS:g} fps, "
        f"clip {WIDTH}x{HEIGHT} at {FPS:g} fps")
    with tempfile.TemporaryDirectory(prefix="video_bench_") as folder:
        clips = write_clips(Path(folder), args.frames)
        for name in args.sources:
            for ssaa in args.ssaa:
                for sink in ("render", "rgb24"):
                    took = {}
                    for sequence in ((False, True) if has_sequence else (False,)):
                        path = "video sequence" if sequence else "frame loop"
                        try:
                            run(clips[name], 30, ssaa, sequence, sink)
                        except (RuntimeError, ValueError) as error:
                            if "other path" in str(error) or "source frames" in str(error):
                                raise
                            say(f"{name:4s} ssaa {ssaa:.0f}x {sink:6s} {path:14s}: not read by this checkout ({type(error).__name__})")
                            continue
                        took[sequence] = min(run(clips[name], args.frames, ssaa, sequence, sink) for _ in range(2))
                        say(f"{name:4s} ssaa {ssaa:.0f}x {sink:6s} {path:14s}: {args.frames} frames in {took[sequence]*1e3:8.1f} ms = "
                            f"{args.frames/took[sequence]:8.1f} frames/s ({took[sequence]/args.frames*1e6:7.1f} us per frame)")
                    if len(took) == 2:
                        say(f"{name:4s} ssaa {ssaa:.0f}x {sink:6s} speed-up {took[False]/took[True]:.2f}x")
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as file:
            file.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
