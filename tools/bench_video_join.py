#!/usr/bin/env python3
"""MusicVideo (examples/scenes.py: a translated fragment that reads iVideo, iSpectrogram and iAudioVolume) at 1920x1080 with a 1920x1080
clip at the scene's rate and a sine sweep, 1x and 2x SSAA: the VideoJoinedSequence (videojoin.py) against the same scene with
SHADERFLOW_VIDEO_JOIN=0, render-only (freewheel, no sink) and rgb24 to /dev/null, from an rgb24 `.npy` clip and from a `.y4m` one, all
in one process. The clips are written into a temporary folder first (`--frames` frames: 6.2 MB each as rgb24, 3.1 MB as 4:2:0). Every
configuration runs once untimed (the fragment's translation and compilation, the contexts, the page cache) and then twice timed; the
faster timed run is reported, under the name of the loop that drew it. GPU box only.

    python tools/bench_video_join.py [--frames 240] [--out profiles/video_join_bench.txt] [--root CHECKOUT] [--tape-loop 0]

`--root`: measure the package of another checkout (the parent commit, for the record in DESIGN §2g) with THIS checkout's scene and
clips. A checkout without the loop draws this single-program scene with the tape loop (tapeloop.py: the video is python logic to it).
`--tape-loop 0` sets SHADERFLOW_TAPE_LOOP=0 for the runs without the loop, so that they are ShaderScene.next's.
"""
import argparse
import importlib.util
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent.parent
WIDTH, HEIGHT, FPS = 1920, 1080, 60.0
LOOPS = (("video_join", "video join"), ("tape_loop", "tape loop"), ("tape_sequence", "tape sequence"), ("video_sequence", "video sequence"))


def own(name: str, path: Path):
    """A module of THIS checkout under a name of its own, beside the measured checkout's package"""
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def write_clips(folder: Path, synth, frames: int) -> dict:
    """The same drifting picture as an rgb24 `.npy` and as a `.y4m` file (its luma the picture's green, flat chroma planes: the reader
    and the kernel move the same bytes whatever they hold)"""
    image = synth.background_image(WIDTH, HEIGHT, seed=3)
    clip = np.lib.format.open_memmap(folder/"clip.npy", mode="w+", dtype=np.uint8, shape=(frames, HEIGHT, WIDTH, 3))
    chroma = np.full(WIDTH*HEIGHT//2, 128, np.uint8).tobytes()
    with open(folder/"clip.y4m", "wb") as file:
        file.write(f"YUV4MPEG2 W{WIDTH} H{HEIGHT} F{int(FPS)}:1 Ip C420jpeg\n".encode())
        for k in range(frames):
            clip[k] = np.roll(image, 3*k, axis=1)
            file.write(b"FRAME\n" + np.ascontiguousarray(clip[k][:, :, 1]).tobytes() + chroma)
    clip.flush()
    return {"npy": folder/"clip.npy", "y4m": folder/"clip.y4m"}


def run(scenes, clip: Path, sound, frames: int, ssaa: float, joined: bool, sink: str, tape_loop: bool) -> tuple:
    os.environ["SHADERFLOW_VIDEO_JOIN"] = "1" if joined else "0"
    os.environ["SHADERFLOW_TAPE_LOOP"] = "1" if (joined or tape_loop) else "0"
    scene = scenes.make(scenes.MusicVideo, audio=(sound, 44100), clip=clip)
    started = time.perf_counter()
    if sink == "render":
        scene.main(width=WIDTH, height=HEIGHT, ssaa=ssaa, fps=FPS, time=frames/FPS, freewheel=True)
    else:
        scene.main(width=WIDTH, height=HEIGHT, ssaa=ssaa, fps=FPS, time=frames/FPS, output="/dev/null")
    took = time.perf_counter() - started
    path = next((label for attribute, label in LOOPS if getattr(scene, attribute, None) is not None), "frame loop")
    if (path == "video join") != joined:
        raise RuntimeError(f"expected {'the video-joined sequence' if joined else 'another loop'}, the scene took the {path}")
    return took, path


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=240)
    p.add_argument("--out", type=Path, default=None, help="the printed lines, appended")
    p.add_argument("--root", type=Path, default=HERE, help="the checkout whose package is measured")
    p.add_argument("--tape-loop", type=int, default=1, help="0: the runs without the loop are ShaderScene.next's")
    args = p.parse_args()
    sys.path.insert(0, str(args.root.resolve()))
    import shaderflow_amd
    from shaderflow_amd import _native
    has_loop = (Path(shaderflow_amd.__file__).parent/"videojoin.py").exists()
    scenes = own("video_join_bench_scenes", HERE/"examples"/"scenes.py")
    synth = own("video_join_bench_synth", HERE/"shaderflow_amd"/"synth.py")
    sound = synth.sweep_clip(args.frames/FPS, 44100)
    lines = []

    def say(line: str) -> None:
        lines.append(line)
        print(line, flush=True)
    say(f"# checkout {'with' if has_loop else 'without'} the video-joined sequence (kernel sources {_native.source_fingerprint()}), MusicVideo, "
        f"{args.frames} frames of {WIDTH}x{HEIGHT} at {FPS:g} fps, a {WIDTH}x{HEIGHT} clip at {FPS:g} fps")
    with tempfile.TemporaryDirectory(prefix="shaderflow-bench-") as folder:
        clips = write_clips(Path(folder), synth, args.frames)
        for source, clip in clips.items():
            for ssaa in (1.0, 2.0):
                for sink in ("render", "rgb24"):
                    took = {}
                    for joined in ((False, True) if has_loop else (False,)):
                        run(scenes, clip, sound, 30, ssaa, joined, sink, bool(args.tape_loop))
                        took[joined], path = min(run(scenes, clip, sound, args.frames, ssaa, joined, sink, bool(args.tape_loop)) for _ in range(2))
                        say(f"{source} ssaa {ssaa:.0f}x {sink:6s} {path:14s}: {args.frames} frames in {took[joined]*1e3:8.1f} ms = "
                            f"{args.frames/took[joined]:8.1f} frames/s ({took[joined]/args.frames*1e6:7.1f} us per frame)")
                    if len(took) == 2:
                        say(f"{source} ssaa {ssaa:.0f}x {sink:6s} speed-up {took[False]/took[True]:.2f}x")
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as file:
            file.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
