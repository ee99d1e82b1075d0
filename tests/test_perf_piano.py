"""
Performance assertion of the piano sequence — `pytest -m perf` on a GPU box, not part of the parity suite (tests/test_perf.py says why).
"""
import os
import time

import pytest

pytestmark = pytest.mark.perf


def test_piano_sequence_is_at_least_twice_the_frame_loop():
    """PianoRoll at 1920x1080, 1x SSAA, render-only: the frame loop pays ShaderPiano.update() on the host and a 512 KB upload of iPianoRoll
    every frame, the sequence one kernel launch. The factor 2 is a floor only a path that still does per-frame host work or per-frame
    uploads would miss (tools/bench_sequences.py measures the gain itself; DESIGN §2d holds the figures); both paths run in this
    process, on this box."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from examples.scenes import PianoRoll
    frames = 600

    def seconds(sequence: bool) -> float:
        os.environ["SHADERFLOW_PIANO_SEQUENCE"] = "1" if sequence else "0"
        best = float("inf")
        for count in (30, frames, frames):                             # one short run untimed: the fragment's compilation, the caches
            scene = PianoRoll()
            started = time.perf_counter()
            scene.main(width=1920, height=1080, ssaa=1.0, fps=60.0, time=count/60.0, freewheel=True)
            took = time.perf_counter() - started
            assert (scene.piano_sequence is not None) == sequence
            if count == frames:
                best = min(best, took)
        return best

    try:
        loop, sequence = seconds(False), seconds(True)
    finally:
        os.environ.pop("SHADERFLOW_PIANO_SEQUENCE", None)
    print({"frame loop": round(frames/loop, 1), "piano sequence": round(frames/sequence, 1), "ratio": round(loop/sequence, 2)})
    assert loop/sequence >= 2.0, (frames/loop, frames/sequence)
