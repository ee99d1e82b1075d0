#!/usr/bin/env python3
"""The five sequence cases (shaderflow_amd/sequence.py: a scene's sources decide the row) against the same scene with the row's flag
switched off, at 1920x1080 and 60 fps, 1x and 2x SSAA, render-only (freewheel, no sink) and rgb24 to /dev/null, all in one process:

    tape        AudioTrails  SHADERFLOW_TAPE_SEQUENCE   two layers, four frames of history, iSpectrogram and iAudioVolume
    piano       PianoRoll    SHADERFLOW_PIANO_SEQUENCE  iPianoKeys, iPianoChan, iPianoRoll, iPianoDynamic
    piano_tape  PianoAudio   SHADERFLOW_PIANO_TAPE      the piano roll with the score's own sound (synth.score_clip)
    video       Video        SHADERFLOW_VIDEO_SEQUENCE  the stock video fragment over a 1920x1080 clip at the scene's rate
    video_join  MusicVideo   SHADERFLOW_VIDEO_JOIN      the same clip with a sine sweep: iVideo, iSpectrogram, iAudioVolume

The scenes are examples/scenes.py's. The video cases read their clip from an rgb24 `.npy` and from a `.y4m` file, written into a temporary
folder first (`--frames` frames: 6.2 MB each as rgb24, 3.1 MB as 4:2:0). Every configuration runs once untimed (the fragment's
translation and compilation, the contexts, the page cache) and then twice timed; the faster timed run is reported, under the name of
the loop that drew it. GPU box only.

    python tools/bench_sequences.py [--cases tape piano …] [--frames 240] [--ssaa 1 2] [--out profiles/sequences_bench.txt] [--root CHECKOUT] [--tape-loop 0]

`--root`: measure the package of another checkout (the parent commit, for the record in profiles/HISTORY.md) with THIS checkout's scenes
and clips. Whether that checkout has a case's loop is seen from the scene after a run: the attribute the run was to be kept under is
set, or the case is reported as drawn by the loop the checkout has for it. `--tape-loop 0` sets SHADERFLOW_TAPE_LOOP=0 for the runs
with the flag off, so that they are ShaderScene.next's and not the tape loop's (tapeloop.py takes a single-program audio scene).
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
# case → the scene of examples/scenes.py, the flag that switches its loop off, the scene attribute its run is kept under
CASES = {"tape": ("AudioTrails", "TAPE_SEQUENCE", "tape_sequence"), "piano": ("PianoRoll", "PIANO_SEQUENCE", "piano_sequence"),
         "piano_tape": ("PianoAudio", "PIANO_TAPE", "piano_tape"), "video": ("Video", "VIDEO_SEQUENCE", "video_sequence"),
         "video_join": ("MusicVideo", "VIDEO_JOIN", "video_join")}
LOOPS = ("video_join", "video_sequence", "piano_tape", "piano_sequence", "tape_sequence", "tape_loop")


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
    # (an `.npy` says no rate: the scenes take it as (frames, fps), memory-mapped as ShaderVideo(path=) would map it)
    return {"npy": (np.load(folder/"clip.npy", mmap_mode="r"), FPS), "y4m": folder/"clip.y4m"}


def run(scenes, case: str, inputs: dict, frames: int, ssaa: float, on: bool, sink: str, tape_loop: bool) -> tuple:
    """(seconds, the loop that drew the scene); with the flag on, a checkout that has the case's loop must have taken it"""
    name, flag, attribute = CASES[case]
    os.environ[f"SHADERFLOW_{flag}"] = "1" if on else "0"
    os.environ["SHADERFLOW_TAPE_LOOP"] = "1" if (on or tape_loop) else "0"
    scene = scenes.make(getattr(scenes, name), **inputs)
    started = time.perf_counter()
    scene.main(width=WIDTH, height=HEIGHT, ssaa=ssaa, fps=FPS, time=frames/FPS, **(dict(freewheel=True) if sink == "render" else dict(output="/dev/null")))
    took = time.perf_counter() - started
    path = next((loop for loop in LOOPS if getattr(scene, loop, None) is not None), "frame_loop")
    if not on and path == attribute:
        raise RuntimeError(f"{case}: SHADERFLOW_{flag}=0, and the scene took {attribute} all the same")
    video = getattr(scene, "video", None)                              # (the clip runs at the scene's rate: every frame shows a new one)
    if video is not None and video._read < frames - 2:
        raise RuntimeError(f"{case}: only {video._read} of {frames} source frames were shown")
    return took, path


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--cases", nargs="*", default=list(CASES), choices=list(CASES))
    p.add_argument("--frames", type=int, default=240)
    p.add_argument("--ssaa", type=float, nargs="*", default=[1.0, 2.0])
    p.add_argument("--out", type=Path, default=None, help="the printed lines, appended")
    p.add_argument("--root", type=Path, default=HERE, help="the checkout whose package is measured")
    p.add_argument("--tape-loop", type=int, default=1, help="0: the runs with the flag off are ShaderScene.next's")
    args = p.parse_args()
    sys.path.insert(0, str(args.root.resolve()))
    from shaderflow_amd import _native
    scenes = own("sequences_bench_scenes", HERE/"examples"/"scenes.py")
    synth = own("sequences_bench_synth", HERE/"shaderflow_amd"/"synth.py")
    seconds = args.frames/FPS
    score = scenes.demo_score(seconds)
    lines = []

    def say(line: str) -> None:
        lines.append(line)
        print(line, flush=True)
    say(f"# checkout {args.root.resolve().name} (kernel sources {_native.source_fingerprint()}), {args.frames} frames of {WIDTH}x{HEIGHT} at {FPS:g} fps")
    with tempfile.TemporaryDirectory(prefix="shaderflow-bench-") as folder:
        clips = write_clips(Path(folder), synth, args.frames) if {"video", "video_join"} & set(args.cases) else {}
        sweep = (synth.sweep_clip(seconds + 1.0, 44100), 44100)
        inputs = {"tape": {"": dict(audio=sweep)}, "piano": {"": dict(score=score)},
                  "piano_tape": {"": dict(score=score, audio=(synth.score_clip(score, seconds), 44100))},
                  "video": {source: dict(clip=clip) for source, clip in clips.items()},
                  "video_join": {source: dict(clip=clip, audio=sweep) for source, clip in clips.items()}}
        for case in args.cases:
            for source, given in inputs[case].items():
                for ssaa in args.ssaa:
                    for sink in ("render", "rgb24"):
                        label = f"{case:10s} {source:3s} ssaa {ssaa:.0f}x {sink:6s}"
                        took = {}
                        for on in (False, True):
                            _, path = run(scenes, case, given, 30, ssaa, on, sink, bool(args.tape_loop))
                            if on and path != CASES[case][2]:
                                say(f"{label} this checkout has no {CASES[case][2]}: the scene is the {path}'s with the flag on as well")
                                break
                            took[on] = min(run(scenes, case, given, args.frames, ssaa, on, sink, bool(args.tape_loop))[0] for _ in range(2))
                            say(f"{label} {path:14s}: {args.frames} frames in {took[on]*1e3:8.1f} ms = "
                                f"{args.frames/took[on]:8.1f} frames/s ({took[on]/args.frames*1e6:7.1f} us per frame)")
                        if len(took) == 2:
                            say(f"{label} speed-up {took[False]/took[True]:.2f}x")
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as file:
            file.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
