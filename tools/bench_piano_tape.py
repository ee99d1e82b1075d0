#!/usr/bin/env python3
"""PianoAudio (examples/scenes.py: a translated fragment that reads iPianoKeys, iPianoChan, iPianoRoll, iPianoDynamic, iSpectrogram and
iAudioVolume) at 1920x1080, 1x and 2x SSAA, with the score's own sound (synth.score_clip): the PianoTapeSequence (pianotape.py) against
the same scene with SHADERFLOW_PIANO_TAPE=0, render-only (freewheel, no sink) and rgb24 to /dev/null, all in one process. Every
configuration runs once untimed (the fragment's translation and compilation, the contexts, the caches) and then twice timed; the
faster timed run is reported, under the name of the loop that drew it. GPU box only.

    python tools/bench_piano_tape.py [--frames 600] [--out profiles/piano_tape_bench.txt] [--root CHECKOUT] [--tape-loop 0]

`--root`: measure the package of another checkout (the parent commit, for the record in DESIGN §2f) with THIS checkout's scene and clip.
A checkout without the sequence draws the scene with the loop it has for it. `--tape-loop 0` sets SHADERFLOW_TAPE_LOOP=0 for the runs
without the sequence, so that they are ShaderScene.next's and not the tape loop's (tapeloop.py takes a single-program scene of this kind).
"""
import argparse
import importlib.util
import os
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent
WIDTH, HEIGHT, FPS = 1920, 1080, 60.0


def own(name: str, path: Path):
    """A module of THIS checkout under a name of its own, beside the measured checkout's package"""
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def run(scenes, clip, frames: int, ssaa: float, sequence: bool, sink: str, tape_loop: bool) -> tuple:
    os.environ["SHADERFLOW_PIANO_TAPE"] = "1" if sequence else "0"
    os.environ["SHADERFLOW_TAPE_LOOP"] = "1" if (sequence or tape_loop) else "0"
    scene = scenes.make(scenes.PianoAudio, score=scenes.demo_score(frames/FPS), audio=(clip, 44100))
    started = time.perf_counter()
    if sink == "render":
        scene.main(width=WIDTH, height=HEIGHT, ssaa=ssaa, fps=FPS, time=frames/FPS, freewheel=True)
    else:
        scene.main(width=WIDTH, height=HEIGHT, ssaa=ssaa, fps=FPS, time=frames/FPS, output="/dev/null")
    took = time.perf_counter() - started
    path = next((label for attribute, label in (("piano_tape", "piano tape"), ("tape_loop", "tape loop"), ("tape_sequence", "tape sequence"),
                                                ("piano_sequence", "piano sequence")) if getattr(scene, attribute, None) is not None), "frame loop")
    if (path == "piano tape") != sequence:
        raise RuntimeError(f"expected {'the piano tape sequence' if sequence else 'another loop'}, the scene took the {path}")
    return took, path


def main() -> None:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, default=600)
    p.add_argument("--out", type=Path, default=None, help="the printed lines, appended")
    p.add_argument("--root", type=Path, default=HERE, help="the checkout whose package is measured")
    p.add_argument("--tape-loop", type=int, default=1, help="0: the runs without the sequence are ShaderScene.next's")
    args = p.parse_args()
    sys.path.insert(0, str(args.root.resolve()))
    import shaderflow_amd
    from shaderflow_amd import _native
    has_sequence = (Path(shaderflow_amd.__file__).parent/"pianotape.py").exists()
    scenes = own("piano_tape_bench_scenes", HERE/"examples"/"scenes.py")
    clip = own("piano_tape_bench_synth", HERE/"shaderflow_amd"/"synth.py").score_clip(scenes.demo_score(args.frames/FPS), args.frames/FPS)
    lines = []

    def say(line: str) -> None:
        lines.append(line)
        print(line, flush=True)
    say(f"# checkout {'with' if has_sequence else 'without'} the piano tape sequence (kernel sources {_native.source_fingerprint()}), PianoAudio, "
        f"{args.frames} frames of {WIDTH}x{HEIGHT} at {FPS:g} fps")
    for ssaa in (1.0, 2.0):
        for sink in ("render", "rgb24"):
            took = {}
            for sequence in ((False, True) if has_sequence else (False,)):
                run(scenes, clip, 30, ssaa, sequence, sink, bool(args.tape_loop))
                took[sequence], path = min(run(scenes, clip, args.frames, ssaa, sequence, sink, bool(args.tape_loop)) for _ in range(2))
                say(f"ssaa {ssaa:.0f}x {sink:6s} {path:14s}: {args.frames} frames in {took[sequence]*1e3:8.1f} ms = "
                    f"{args.frames/took[sequence]:8.1f} frames/s ({took[sequence]/args.frames*1e6:7.1f} us per frame)")
            if len(took) == 2:
                say(f"ssaa {ssaa:.0f}x {sink:6s} speed-up {took[False]/took[True]:.2f}x")
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as file:
            file.write("".join(line + "\n" for line in lines))


if __name__ == "__main__":
    main()
