#!/usr/bin/env python3
"""AudioTrails (examples/scenes.py: translated fragment, two layers, four frames of history, iSpectrogram and iAudioVolume) at 1920x1080,
1x and 2x SSAA: the frame loop (SHADERFLOW_TAPE_SEQUENCE=0: scene.next per frame, host audio per frame) against the TapeSequence
(tapesequence.py), render-only (freewheel, no sink) and rgb24 to /dev/null, all in one process. Every configuration runs once untimed
(the fragment's translation and compilation, the contexts, the caches) and then twice timed; the faster timed run is reported.
GPU box only.

    python tools/bench_tape_sequence.py [--frames 600] [--out profiles/tape_sequence_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import examples.scenes as scenes  # noqa: E402
from shaderflow_amd import synth  # noqa: E402


def run(frames: int, ssaa: float, sequence: bool, sink: str, clip) -> float:
    os.environ["SHADERFLOW_TAPE_SEQUENCE"] = "1" if sequence else "0"
    scene = scenes.make(scenes.AudioTrails, audio=(clip, 44100))
    started = time.perf_counter()
    if sink == "render":
        scene.main(width=1920, height=1080, ssaa=ssaa, fps=60.0, time=frames/60.0, freewheel=True)
    else:
        scene.main(width=1920, height=1080, ssaa=ssaa, fps=60.0, time=frames/60.0, output="/dev/null")
    took = time.perf_counter() - started
    if (scene.tape_sequence is not None) != sequence:
        raise RuntimeError(f"expected the {'tape sequence' if sequence else 'frame loop'}, the scene took the other path")
    return took


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=600)
    p.add_argument("--out", type=Path, default=None, help="JSON lines of the results")
    args = p.parse_args()
    clip = synth.sweep_clip(args.frames/60.0 + 1.0, 44100)
    rows = []
    for ssaa in (1.0, 2.0):
        for sink in ("render", "rgb24"):
            for sequence in (False, True):
                run(30, ssaa, sequence, sink, clip)
                took = min(run(args.frames, ssaa, sequence, sink, clip) for _ in range(2))
                row = {"scene": "AudioTrails", "width": 1920, "height": 1080, "ssaa": ssaa, "sink": sink,
                       "path": "tape sequence" if sequence else "frame loop", "frames": args.frames, "seconds": round(took, 4),
                       "frames_per_second": round(args.frames/took, 1), "us_per_frame": round(took/args.frames*1e6, 1)}
                rows.append(row)
                print(f"ssaa {ssaa:.0f}x {sink:6s} {row['path']:13s}: {args.frames} frames in {took*1e3:8.1f} ms = "
                      f"{row['frames_per_second']:8.1f} frames/s ({row['us_per_frame']:7.1f} us per frame)", flush=True)
            loop, tape = rows[-2], rows[-1]
            print(f"ssaa {ssaa:.0f}x {sink:6s} speed-up {loop['seconds']/tape['seconds']:.2f}x", flush=True)
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("".join(json.dumps(row) + "\n" for row in rows))


if __name__ == "__main__":
    main()
