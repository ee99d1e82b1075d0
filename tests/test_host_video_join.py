"""
The host halves of the video-joined sequence (shaderflow_amd/sequence.py) that need no device: `clockloop.JoinedSource` with THREE parts
that record their calls — the piano, the tape that cuts the run, and last the video that shortens calls — the `video_join` field of the
sequence descriptor, the translator's sampler slots beside the two the tape replaces, and `video_fits`.
"""
from __future__ import annotations

import ctypes as C
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from shaderflow_amd.clockloop import FrameSource, JoinedSource

ROOT = Path(__file__).resolve().parent.parent


class Part(FrameSource):
    """A frame source that writes every call into a shared log"""

    def __init__(self, name, log, shorten=None, settle_error=None):
        self.name, self.log, self.shorten, self.settle_error = name, log, shorten, settle_error

    def prepare(self, times, dts, total): self.log.append((self.name, "prepare", total))
    def begin_batch(self, first, size): self.log.append((self.name, "begin_batch", first, size))
    def attach(self, sequence): self.log.append((self.name, "attach"))
    def consumed(self, first, count): self.log.append((self.name, "consumed", first, count))
    def release(self): self.log.append((self.name, "release"))

    def take(self, sequence, first, count, batch_first):
        self.log.append((self.name, "take", first, count, batch_first))
        return count if self.shorten is None else min(count, self.shorten)

    def settle(self, done):
        self.log.append((self.name, "settle", done))
        if self.settle_error is not None:
            raise self.settle_error

    def finished(self, done, total):
        self.log.append((self.name, "finished", done, total))
        return True


class Cutting(Part):
    def batches(self, total):
        self.log.append((self.name, "batches", total))
        return [(first, min(60, total - first)) for first in range(0, total, 60)]


def three(log, **video):
    return JoinedSource([Part("piano", log), Cutting("tape", log), Part("video", log, **video)], end="next", chunked=True)


def test_every_method_reaches_the_three_parts_in_order():
    log = []
    joined = three(log, shorten=4)
    assert (joined.end, joined.chunked) == ("next", True)
    joined.prepare([0.0], [0.0], 130)
    assert joined.batches(130) == [(0, 60), (60, 60), (120, 10)]
    joined.attach(SimpleNamespace())
    joined.begin_batch(60, 60)
    assert joined.take(SimpleNamespace(), 66, 30, 60) == 4              # the last part shortens the call: accepted
    joined.consumed(66, 4)
    joined.settle(70)
    assert joined.finished(70, 130)
    joined.release()
    names = ("piano", "tape", "video")
    assert log == [*((n, "prepare", 130) for n in names), ("tape", "batches", 130), *((n, "attach") for n in names),
                   *((n, "begin_batch", 60, 60) for n in names), *((n, "take", 66, 30, 60) for n in names),
                   *((n, "consumed", 66, 4) for n in names), *((n, "settle", 70) for n in names), *((n, "finished", 70, 130) for n in names),
                   *((n, "release") for n in reversed(names))]


def test_a_shortening_part_in_front_of_another_trips_the_assertion():
    log = []
    joined = JoinedSource([Part("piano", log), Part("video", log, shorten=4), Cutting("tape", log)])
    with pytest.raises(AssertionError, match="Part.take shortened the call to 4 of 30"):
        joined.take(SimpleNamespace(), 66, 30, 60)
    assert not any(entry[:2] == ("tape", "take") for entry in log)


def test_two_cutting_parts_are_refused():
    with pytest.raises(ValueError, match="2 frame sources cut the run"):
        JoinedSource([Cutting("tape", []), Part("piano", []), Cutting("other", [])])


def test_settle_reaches_all_three_and_raises_the_first_error_again():
    log = []
    first, second = OSError("the reader"), RuntimeError("the device")
    joined = JoinedSource([Part("piano", log, settle_error=first), Cutting("tape", log), Part("video", log, settle_error=second)])
    with pytest.raises(OSError) as raised:
        joined.settle(40)
    assert raised.value is first
    assert log == [("piano", "settle", 40), ("tape", "settle", 40), ("video", "settle", 40)]


# ---- the descriptor ------------------------------------------------------------------------------------------------------------------

def test_video_join_is_the_descriptors_last_field_and_zero_by_default():
    from shaderflow_amd import _native as N
    names = [name for name, _ in N.Sequence._fields_]
    assert names[-1] == "video_join" and names[-2] == "video_names"
    assert N.Sequence.video_join.size == 4
    # the field offset arithmetic of the C struct: an int32 right behind the last pointer, the whole padded to the pointers' alignment
    assert N.Sequence.video_join.offset == N.Sequence.video_names.offset + C.sizeof(C.c_void_p)
    assert C.sizeof(N.Sequence) == -(-(N.Sequence.video_join.offset + 4)//C.alignment(C.c_void_p))*C.alignment(C.c_void_p)
    assert N.Sequence().video_join == 0 and N.Sequence(video=N.Handle(1), tape=N.Handle(1)).video_join == 0


def test_the_ctypes_descriptor_is_the_headers_struct(tmp_path):
    """sizeof and the offsets of the three optional parts, from the header itself through the host compiler (the one build() compiles
    the oracle with)"""
    from shaderflow_amd import _native as N
    compiler = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert compiler, "no host C compiler: build() needs one as well"
    fields = ("tape", "tape_frame0", "piano", "piano_ticks", "video", "video_slots", "video_names", "video_join")
    prints = "".join(f'    printf("{name} %zu\\n", offsetof(sfx_sequence, {name}));\n' for name in fields)
    (tmp_path/"layout.c").write_text('#include <stddef.h>\n#include <stdio.h>\n#include "shaderflow_hip.h"\nint main(void) {\n'
                                     '    printf("sizeof %zu\\n", sizeof(sfx_sequence));\n' + prints + "    return 0;\n}\n")
    subprocess.run([compiler, "-I", str(ROOT/"include"), "-o", str(tmp_path/"layout"), str(tmp_path/"layout.c")], check=True)
    out = dict(line.split() for line in subprocess.run([str(tmp_path/"layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == C.sizeof(N.Sequence)
    for name in fields:
        assert int(out[name]) == getattr(N.Sequence, name).offset, name


# ---- the sampler slots the tape replaces ---------------------------------------------------------------------------------------------------

SLOTS_FRAGMENT = """
    void main() {
        vec3 clip = texture(iVideo, astuv).rgb + texture(iVideo2x0, astuv).rgb;
        vec2 s = texture(iSpectrogram, vec2(0.5, astuv.x)).xy;
        vec2 w = texture(iWaveform, vec2(astuv.x, 0.0)).xy;
        fragColor = vec4(clip*s.x*w.x + texture(other, astuv).rgb, 1.0);
    }
"""


@pytest.mark.parametrize("order", ["video-first", "audio-first"])
def test_a_translated_fragment_never_puts_the_video_into_the_tapes_slots(order):
    """glsl2hip hands sampler slots 1 and 2 to iSpectrogram and iWaveform alone, wherever they stand in the pipeline: every row name of a
    temporal video and any other texture gets one of the free slots — what lets `bind_tape` replace the two under a video's feet"""
    from shaderflow_amd import glsl2hip
    video = [("sampler2D", f"iVideo{depth}x0") for depth in range(3)]
    audio = [("sampler2D", "iSpectrogram0x0"), ("sampler2D", "iWaveform0x0")]
    pipeline = [*video, ("sampler2D", "other0x0"), *audio] if order == "video-first" else [*audio, *video, ("sampler2D", "other0x0")]
    defines = "".join(f"#define {name[:-3]} {name}\n" for _, name in (video[0], *audio, ("sampler2D", "other0x0")))
    translation = glsl2hip.translate(defines + SLOTS_FRAGMENT, pipeline)
    slots = {binding.name: binding.slot for binding in translation.bindings if binding.type == "sampler2D"}
    assert slots["iSpectrogram0x0"] == 1 and slots["iWaveform0x0"] == 2 == glsl2hip.FIXED_SAMPLER_SLOTS["iWaveform"]
    assert {"iVideo0x0", "iVideo2x0", "other0x0"} <= set(slots)
    for name, slot in slots.items():
        if not name.startswith(("iSpectrogram", "iWaveform")):
            assert slot not in (1, 2), (name, slot)
    assert len(set(slots.values())) == len(slots)


# ---- video_fits ----------------------------------------------------------------------------------------------------------------------------

def texture(**fields):
    box = SimpleNamespace(texture=object())
    values = dict(layers=1, components=3, dtype=np.dtype(np.uint8), track=0.0, size=(64, 36), boxes=[(0, 0, box)])
    values.update(fields)
    return SimpleNamespace(**values)


def test_video_fits_is_the_texture_half_of_the_video_sequences_answer():
    """The conditions VideoSequence.applicable asked of the texture before the extraction, one at a time (test_gpu_video.py's fallback
    scenes: `two-layers`), on stand-ins that need no device"""
    from shaderflow_amd.videosequence import video_fits
    video = lambda **fields: SimpleNamespace(width=64, height=36, texture=texture(**fields))       # noqa: E731
    assert video_fits(video())
    assert not video_fits(SimpleNamespace(width=64, height=36, texture=None))
    assert not video_fits(video(layers=2))
    assert not video_fits(video(components=4))
    assert not video_fits(video(dtype=np.dtype(np.float32)))
    assert not video_fits(video(track=1.0))
    assert not video_fits(video(size=(32, 18)))
    assert not video_fits(video(boxes=[(0, 0, SimpleNamespace(texture=object())), (1, 0, SimpleNamespace(texture=None))]))


def test_the_video_sequence_asks_video_fits(monkeypatch):
    """Sequence.applicable for a video alone is the gate and then video_fits, for the same video: the video's answer is the same
    function alone and in a join"""
    from shaderflow_amd import sequence, videosequence
    from shaderflow_amd.video import ShaderVideo
    assert sequence.video_fits is videosequence.video_fits
    asked = []
    video = object.__new__(ShaderVideo)                                 # (no device: the fields video_fits and the gate's caller read)
    video.name, video.width, video.height, video.texture = "iVideo", 64, 36, texture()
    scene = SimpleNamespace(modules=[video])
    monkeypatch.setattr(sequence, "sequence_gate", lambda scene, export, turbo, taped, chunked: asked.append(list(taped)) or True)
    assert sequence.Sequence.applicable(scene) is True and sequence.Sequence.taken(scene) == "video_sequence"
    del asked[1:]
    video.texture.layers = 2
    assert sequence.Sequence.applicable(scene) is False
    monkeypatch.setattr(sequence, "sequence_gate", lambda *args, **kwargs: False)
    assert sequence.Sequence.applicable(scene) is False
    assert asked == [[video, video.texture], [video, video.texture]]
