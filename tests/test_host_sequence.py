"""
The table of `shaderflow_amd/sequence.py` as data, for every non-empty set of sources a scene can have (piano, tape, video): the scene
attribute, the flags, the clock behind the run, `chunked`, the order of the parts, `video_join` in the descriptor, what is handed to
the gate, and every flag's switch — on stand-in modules that need no device.
"""
from __future__ import annotations

from itertools import combinations
from types import SimpleNamespace

from shaderflow_amd.clockloop import FrameSource


def stand_ins():
    """One module of every stock type as the bare object (no device, no scene), with the fields `Sequence.taken` reads before the fits"""
    from shaderflow_amd.audio.module import ShaderAudio
    from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
    from shaderflow_amd.audio.waveform import ShaderWaveform
    from shaderflow_amd.piano.module import ShaderPiano
    from shaderflow_amd.video import ShaderVideo
    piano, audio, video = object.__new__(ShaderPiano), object.__new__(ShaderAudio), object.__new__(ShaderVideo)
    piano.keys_texture, piano.channel_texture, piano.roll_texture, piano.tempo_texture = (SimpleNamespace(name=name) for name in "kcrt")
    audio.volume, audio.std = SimpleNamespace(name="volume"), SimpleNamespace(name="std")
    video.name, video.texture = "iVideo", SimpleNamespace(name="iVideo")
    spectrogram, waveform = object.__new__(ShaderSpectrogram), object.__new__(ShaderWaveform)
    handed = {"piano": [piano, piano.keys_texture, piano.channel_texture, piano.roll_texture, piano.tempo_texture],
              "tape": [audio, spectrogram, waveform, audio.volume, audio.std], "video": [video, video.texture]}
    modules = {"piano": [piano], "tape": [audio, spectrogram, waveform], "video": [video]}
    return modules, handed


class StandInPart(FrameSource):
    def __init__(self, kind, clock):
        self.kind, self.clock = kind, clock


WANT = {                                                                # kinds → attribute, flags, end, chunked
    ("video",): ("video_sequence", {"VIDEO_SEQUENCE"}, "next", True),
    ("piano",): ("piano_sequence", {"PIANO_SEQUENCE"}, "next", True),
    ("tape",): ("tape_sequence", {"TAPE_SEQUENCE"}, "last_dt", False),
    ("piano", "tape"): ("piano_tape", {"PIANO_SEQUENCE", "TAPE_SEQUENCE", "PIANO_TAPE"}, "next", True),
    ("piano", "video"): ("video_join", {"PIANO_SEQUENCE", "VIDEO_SEQUENCE", "VIDEO_JOIN"}, "next", True),
    ("tape", "video"): ("video_join", {"TAPE_SEQUENCE", "VIDEO_SEQUENCE", "VIDEO_JOIN"}, "next", True),
    ("piano", "tape", "video"): ("video_join", {"PIANO_SEQUENCE", "TAPE_SEQUENCE", "VIDEO_SEQUENCE", "VIDEO_JOIN"}, "next", True),
}


def test_the_table_says_for_every_set_of_sources_what_the_five_loops_said(monkeypatch):
    from shaderflow_amd import _native as N
    from shaderflow_amd import sequence
    from shaderflow_amd.sequence import KINDS, ROWS, Sequence, flags
    assert KINDS == ("piano", "tape", "video")
    every = [kinds for size in (1, 2, 3) for kinds in combinations(KINDS, size)]
    assert set(every) == set(WANT) and set(ROWS) == {frozenset(kinds) for kinds in every}
    gated = []

    def gate(scene, export, turbo, taped, chunked):
        gated.append((export, turbo, list(taped), chunked))
        return True
    monkeypatch.setattr(sequence, "sequence_gate", gate)
    for name in ("piano_fits", "video_fits", "camera_at_identity"):
        monkeypatch.setattr(sequence, name, lambda *args: True)
    monkeypatch.setattr(sequence.FrameTape, "audio_fits", staticmethod(lambda *args: True))
    # the parts and the clock as recording stand-ins: what a Sequence builds of them, in which order, and what `attach` adds
    monkeypatch.setattr(sequence, "ClockLoop", lambda scene: SimpleNamespace(scene=scene))
    for kind, name in zip(KINDS, ("PianoSequence", "TapeSequence", "VideoSequence")):
        monkeypatch.setattr(sequence, name, lambda scene, *clock, kind=kind: StandInPart(kind, clock))
    for flag in set().union(*(row[1] for row in WANT.values())):
        monkeypatch.delenv(f"SHADERFLOW_{flag}", raising=False)
    export = SimpleNamespace(mjpeg=False, relay=None)

    for kinds in every:
        attribute, switches, end, chunked = WANT[kinds]
        row = ROWS[frozenset(kinds)]
        assert (row.attribute, set(flags(kinds)), row.end, row.chunked) == (attribute, switches, end, chunked), kinds
        assert len(flags(kinds)) == len(switches)
        modules, handed = stand_ins()
        scene = SimpleNamespace(modules=["the scene", *(m for kind in reversed(kinds) for m in modules[kind])])

        # what goes to the gate: the union of the parts' own, once; the tape alone is asked without the export and not chunked
        del gated[:]
        assert Sequence.taken(scene, export, False) == attribute and Sequence.applicable(scene, export, False) is True
        assert len(gated) == 2 and gated[0][2:] == gated[1][2:]
        asked_export, turbo, taped, asked_chunked = gated[0]
        want = [m for kind in kinds for m in handed[kind]]
        assert len(taped) == len(want) and {id(m) for m in taped} == {id(m) for m in want}, kinds
        assert (asked_export, turbo, asked_chunked) == ((export if chunked else None), False, chunked)

        # every flag of the row switches the sequence off on its own, and no other flag does
        for flag in switches:
            monkeypatch.setenv(f"SHADERFLOW_{flag}", "0")
            assert Sequence.applicable(scene, export) is False and Sequence.taken(scene, export) is None, (kinds, flag)
            monkeypatch.setenv(f"SHADERFLOW_{flag}", "1")
            assert Sequence.applicable(scene, export) is True
            monkeypatch.delenv(f"SHADERFLOW_{flag}")
        for flag in set().union(*(row[1] for row in WANT.values())) - switches:
            monkeypatch.setenv(f"SHADERFLOW_{flag}", "0")
            assert Sequence.taken(scene, export) == attribute, (kinds, flag)
            monkeypatch.delenv(f"SHADERFLOW_{flag}")

        # the loop: one clock, the parts in the order piano, tape, video, the video with the shared clock, the row's end and chunked
        loop = Sequence(scene)
        assert [part.kind for part in loop.parts] == list(kinds) and loop.row is row
        assert (loop.end, loop.chunked, loop.frames) == (end, chunked, 0)
        for kind, part in zip(KINDS, (loop.piano, loop.tape, loop.video)):
            assert (part is not None) == (kind in kinds) and (part is None or part.kind == kind)
        assert loop.clock.scene is scene
        assert loop.video is None or (len(loop.video.clock) == 1 and loop.video.clock[0] is loop.clock)
        assert loop.piano is None or loop.piano.clock == ()             # (PianoSequence(scene) stands on its own)
        descriptor = N.Sequence()
        loop.attach(descriptor)
        assert descriptor.video_join == (1 if "video" in kinds and len(kinds) > 1 else 0), kinds

    # a second or a subclassed piano or video refuses the scene before the gate is asked; without any source there is no row
    from shaderflow_amd.video import ShaderVideo
    modules, _ = stand_ins()
    del gated[:]
    assert Sequence.taken(SimpleNamespace(modules=[*modules["video"], *stand_ins()[0]["video"]]), export) is None
    assert Sequence.taken(SimpleNamespace(modules=[object.__new__(type("Subclassed", (ShaderVideo,), {}))]), export) is None
    assert Sequence.taken(SimpleNamespace(modules=["the scene"]), export) is None and not gated
