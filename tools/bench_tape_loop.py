"""
Frames per second of an audio scene with update() logic of its own (tests/test_gpu_tape_loop.py's counting Visualizer) at 3840x2160,
2x SSAA: the frame loop (batch=False) against TapeLoop (batch=None), render only (freewheel, no output) and rgb24 frames read out to
the host and written to /dev/null (the raw-file sink, as bench.py's export figure).
Prints one JSON line.

    python tools/bench_tape_loop.py [--frames 600] [--width 3840 --height 2160 --ssaa 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--frames", type=int, default=600)
    parser.add_argument("--width", type=int, default=3840)
    parser.add_argument("--height", type=int, default=2160)
    parser.add_argument("--ssaa", type=float, default=2.0)
    parser.add_argument("--profile", type=str, default=None, help="write a cProfile of one TapeLoop render-only run here")
    args = parser.parse_args()

    from examples.scenes import Visualizer
    from shaderflow_amd import synth

    class Counting(Visualizer):
        audio_source = (synth.sweep_clip(args.frames/60.0 + 1.0, 44100), 44100)
        background = synth.background_image(1920, 1080, seed=3)
        counted = 0

        def update(self):
            self.counted += 1

    def run(batch, output):
        scene = Counting()
        kwargs = dict(width=args.width, height=args.height, fps=60.0, ssaa=args.ssaa, subsample=2, batch=batch)
        scene.main(**kwargs, time=4/60.0, output=output, freewheel=output is None)          # warm-up: compile, allocate
        started = time.perf_counter()
        scene.main(**kwargs, time=args.frames/60.0, output=output, freewheel=output is None)
        took = time.perf_counter() - started
        assert scene.counted == args.frames + 4
        path = "tape_loop" if scene.tape_loop is not None else "frame_loop"
        return round(args.frames/took, 1), path

    result = {"scene": "Visualizer+update()", "width": args.width, "height": args.height, "ssaa": args.ssaa, "frames": args.frames}
    for name, batch, output in (("frame_loop_render", False, None), ("tape_loop_render", None, None),
                                ("frame_loop_rgb24", False, os.devnull), ("tape_loop_rgb24", None, os.devnull)):
        fps, path = run(batch, output)
        result[name] = fps
        result[name + "_path"] = path
    if args.profile:
        import cProfile
        import pstats
        scene = Counting()
        kwargs = dict(width=args.width, height=args.height, fps=60.0, ssaa=args.ssaa, subsample=2, batch=None, freewheel=True)
        scene.main(**kwargs, time=4/60.0)
        profiler = cProfile.Profile()
        profiler.enable()
        scene.main(**kwargs, time=60/60.0)
        profiler.disable()
        with open(args.profile, "w") as out:
            pstats.Stats(profiler, stream=out).sort_stats("tottime").print_stats(30)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
