#!/usr/bin/env python3
"""PianoRoll (examples/scenes.py: translated fragment that reads iPianoKeys, iPianoChan, iPianoRoll and iPianoDynamic) at 1920x1080, 1x and
2x SSAA: the frame loop (SHADERFLOW_PIANO_SEQUENCE=0: scene.next per frame, ShaderPiano.update() and its three texture uploads on the
host) against the PianoSequence (pianosequence.py), render-only (freewheel, no sink) and rgb24 to /dev/null, all in one process. Every
configuration runs once untimed (the fragment's translation and compilation, the contexts, the caches) and then twice timed; the
faster timed run is reported. GPU box only.

    python tools/bench_piano_sequence.py [--frames 600] [--out profiles/piano_sequence_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import examples.scenes as scenes  # noqa: E402


def run(frames: int, ssaa: float, sequence: bool, sink: str) -> float:
    os.environ["SHADERFLOW_PIANO_SEQUENCE"] = "1" if sequence else "0"
    scene = scenes.make(scenes.PianoRoll, score=scenes.demo_score(frames/60.0))
    started = time.perf_counter()
    if sink == "render":
        scene.main(width=1920, height=1080, ssaa=ssaa, fps=60.0, time=frames/60.0, freewheel=True)
    else:
        scene.main(width=1920, height=1080, ssaa=ssaa, fps=60.0, time=frames/60.0, output="/dev/null")
    took = time.perf_counter() - started
    if (scene.piano_sequence is not None) != sequence:
        raise RuntimeError(f"expected the {'piano sequence' if sequence else 'frame loop'}, the scene took the other path")
    return took


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=600)
    p.add_argument("--out", type=Path, default=None, help="JSON lines of the results")
    args = p.parse_args()
    rows = []
    for ssaa in (1.0, 2.0):
        for sink in ("render", "rgb24"):
            for sequence in (False, True):
                run(30, ssaa, sequence, sink)
                took = min(run(args.frames, ssaa, sequence, sink) for _ in range(2))
                row = {"scene": "PianoRoll", "width": 1920, "height": 1080, "ssaa": ssaa, "sink": sink,
                       "path": "piano sequence" if sequence else "frame loop", "frames": args.frames, "seconds": round(took, 4),
                       "frames_per_second": round(args.frames/took, 1), "us_per_frame": round(took/args.frames*1e6, 1)}
                rows.append(row)
                print(f"ssaa {ssaa:.0f}x {sink:6s} {row['path']:14s}: {args.frames} frames in {took*1e3:8.1f} ms = "
                      f"{row['frames_per_second']:8.1f} frames/s ({row['us_per_frame']:7.1f} us per frame)", flush=True)
            loop, sequence_row = rows[-2], rows[-1]
            print(f"ssaa {ssaa:.0f}x {sink:6s} speed-up {loop['seconds']/sequence_row['seconds']:.2f}x", flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("".join(json.dumps(row) + "\n" for row in rows))


if __name__ == "__main__":
    main()
