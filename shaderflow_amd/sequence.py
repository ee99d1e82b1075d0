"""
Sequence: the frame loop of scenes with a piano, audio modules, a video, or several of them, without python logic (no reference equivalent).

Each source has a part that feeds ClockLoop's native sequence (`sfx_sequence_run`) as a `FrameSource`: `PianoSequence`
(pianosequence.py) puts `k_piano_frame` and the note range in front of every frame's passes, `TapeSequence` (tapesequence.py) builds the
audio state in batches and lets the passes that read audio draw from it, `VideoSequence` (videosequence.py) stages source frames ahead of
the draws and puts `k_video_frame` in front of the frames they land on. This loop is the parts a scene has modules for, as one
`JoinedSource` (clockloop.py) behind one `ClockLoop`: one native call per chunk names all of them. Nothing is computed here that a part
does not compute on its own.

The order of the parts is piano, tape, video. The video goes last because its `take` is the one that shortens a call — to the frames
whose source frames are staged already — and what the parts in front of it set for the call does not depend on the count: the tape sets
`tape_frame0`, where the call starts inside the batch, and the piano the address of the first frame's tick. The tape is the part that
cuts the run into batches; the video shortens calls inside a batch, never across one. A video beside another part says so in the
descriptor (`video_join`: the native call refuses the combination to a caller that does not).

Which sources a scene has decides everything else, and `ROWS` says it once: the `ShaderScene` attribute the run is kept under, the
`SHADERFLOW_<flag>`s that must not be "0" — every part's own and the join's: who switched a half off for an A/B run gets the host's
half — the clock behind the run (`end_clock`) and whether the run is `chunked`. The audio tape alone is the one row that is not
chunked: it also takes a progress relay, a run without turbo and a Motion-JPEG export, frame by frame, and leaves the clock of the
last frame as `FrameTape.export` does. Every other row promises the frame loop's host state of a piano or a video, and that is what
`scene.next` leaves. The audio modules' host state and textures stay what the export found. Behind a run, however it ended, every part
settles its own, and all of them are released.

Out of scope, so they keep the loop they had: python `update()` logic, a subclassed module, several videos or pianos, `layers != 1` on
the video, audio a tape does not compute, a main camera off the identity pose beside audio (`TapeLoop.camera_at_identity` says why),
sharded runs.
"""
from __future__ import annotations

import os
from typing import TYPE_CHECKING, NamedTuple, Optional

import numpy as np

from shaderflow_amd.audio.module import ShaderAudio
from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
from shaderflow_amd.audio.waveform import ShaderWaveform
from shaderflow_amd.clockloop import ClockLoop, JoinedSource
from shaderflow_amd.glsl2hip import FIXED_SAMPLER_SLOTS
from shaderflow_amd.parallel import is_sharded
from shaderflow_amd.piano.module import ShaderPiano
from shaderflow_amd.pianosequence import PianoSequence, piano_fits, piano_textures
from shaderflow_amd.shader import ShaderProgram
from shaderflow_amd.tape import FrameTape
from shaderflow_amd.tapeloop import TapeLoop
from shaderflow_amd.tapesequence import TapeSequence
from shaderflow_amd.video import ShaderVideo
from shaderflow_amd.videosequence import VideoSequence, video_fits

if TYPE_CHECKING:
    from shaderflow_amd.exporting import ExportingHelper
    from shaderflow_amd.scene import ShaderScene

KINDS = ("piano", "tape", "video")                                     # the sources, in the order of their parts
FLAGS = {"piano": "PIANO_SEQUENCE", "tape": "TAPE_SEQUENCE", "video": "VIDEO_SEQUENCE"}


class Row(NamedTuple):
    attribute: str                                                     # the ShaderScene attribute the run is kept under
    join: Optional[str]                                                # the flag of the join itself, beside the parts' FLAGS
    end: str = "next"                                                  # the clock behind the run (end_clock)
    chunked: bool = True                                               # every chunk is ONE native call (sequence_gate saw to it); False: native_sequence is asked


ROWS = {frozenset(kinds): Row(*row) for kinds, *row in (
    (("video",), "video_sequence", None),
    (("piano",), "piano_sequence", None),
    (("tape",), "tape_sequence", None, "last_dt", False),
    (("piano", "tape"), "piano_tape", "PIANO_TAPE"),
    (("piano", "video"), "video_join", "VIDEO_JOIN"),
    (("tape", "video"), "video_join", "VIDEO_JOIN"),
    (("piano", "tape", "video"), "video_join", "VIDEO_JOIN"))}


def flags(kinds) -> tuple:
    """The SHADERFLOW_<flag>s none of which may be "0" for a scene of these kinds to take the sequence"""
    return (*(FLAGS[kind] for kind in KINDS if kind in kinds), *filter(None, (ROWS[frozenset(kinds)].join,)))


def sources(scene: "ShaderScene") -> tuple:
    """(kind → the scene's modules of it, the kinds it has any of: its key in ROWS). A piano and a video are whatever `isinstance` finds: a subclass (which may update() differently
    from what the device computes) or a second one refuses the scene. The tape's are the ShaderAudio of the exact type: a subclass is
    left to ClockLoop's judgement, which refuses it."""
    found = {"piano": [m for m in scene.modules if isinstance(m, ShaderPiano)], "tape": [m for m in scene.modules if type(m) is ShaderAudio],
             "video": [m for m in scene.modules if isinstance(m, ShaderVideo)]}
    return found, frozenset(kind for kind in KINDS if found[kind])


def sequence_gate(scene: "ShaderScene", export: "Optional[ExportingHelper]", turbo: bool, taped, chunked: bool) -> bool:
    """What every row asks of the scene: a freewheel run that is not sharded, to a sink sfx_sequence_run knows; when the loop is `chunked`
    turbo, no progress relay and every program compiled; everything but the modules `taped` is what ClockLoop takes: no python logic, no
    other module type"""
    if not scene.freewheel or is_sharded():
        return False
    if export is not None and export.sized:                         # a sized-frame format (mjpeg, png). sfx_sequence_run's own sink knows rgb24 and yuv420p: the loop from before the sequences draws
        return False
    if chunked and (not turbo or (export is not None and export.relay is not None)):
        return False
    if not ClockLoop.applicable(scene, taped=frozenset(id(m) for m in taped)):
        return False
    return not chunked or all(m.program is not None for m in scene.modules if isinstance(m, ShaderProgram))


def camera_at_identity(scene: "ShaderScene") -> bool:
    """Whether the camera uniforms the modules yield are the identity pose's (TapeLoop.IDENTITY, compared as the float32 / int32
    values a push would send). The camera cannot move here (ClockLoop.applicable), so its pose before the first frame is its pose."""
    seen = {}
    for module in scene.modules:
        if module is scene:
            continue
        for variable in module.pipeline() or ():
            if variable.name in TapeLoop.IDENTITY:
                seen[variable.name] = variable.value
    for name, (dtype, want) in TapeLoop.IDENTITY.items():
        if name not in seen or seen[name] is None:
            continue
        value = seen[name]
        value = getattr(value, "value", value)                    # (an enum: its number)
        if not np.array_equal(np.asarray(value, dtype=np.float64).astype(dtype).reshape(-1)[:len(want)], np.asarray(want, dtype)):
            return False
    return True


class Sequence(JoinedSource):
    @staticmethod
    def taken(scene: "ShaderScene", export: "ExportingHelper | None" = None, turbo: bool = True) -> Optional[str]:
        """The attribute of the row (ROWS) this scene's run is kept under; None for a scene that is not a sequence's"""
        found, kinds = sources(scene)
        if not kinds or any(os.environ.get(f"SHADERFLOW_{flag}", "1") == "0" for flag in flags(kinds)):
            return None
        if any(len(found[kind]) != 1 or type(found[kind][0]) is not exact for kind, exact in (("piano", ShaderPiano), ("video", ShaderVideo)) if kind in kinds):
            return None
        row, audios = ROWS[kinds], found["tape"]
        piano, video = (found[kind][0] if kind in kinds else None for kind in ("piano", "video"))
        # what the parts compute for the caller, so ClockLoop's judgement leaves it alone: the piano and its textures, the video and its
        # texture, and beside a ShaderAudio the audio modules of exact stock types with the two loudness systems each audio owns
        taped = [*(piano_textures(piano) if piano is not None else ()), *((video, video.texture) if video is not None else ())]
        if audios:
            spectrograms = [m for m in scene.modules if type(m) is ShaderSpectrogram]
            waveforms = [m for m in scene.modules if type(m) is ShaderWaveform]
            taped += (*audios, *spectrograms, *waveforms, *(s for a in audios for s in (a.volume, a.std)))
        # (the tape alone is asked without the export: a relay, a run without turbo and a Motion-JPEG sink go frame by frame, `pipe_here`)
        if not sequence_gate(scene, export if row.chunked else None, turbo, taped, row.chunked):
            return None
        if (piano is not None and not piano_fits(piano)) or (video is not None and not video_fits(video)):
            return None
        if audios and not (FrameTape.audio_fits(audios, spectrograms, waveforms) and camera_at_identity(scene)):
            return None
        # a video that goes by one of the two sampler names the tape replaces per frame would lose its slot to the tape (the native
        # call refuses such a descriptor)
        if audios and video is not None and video.name in FIXED_SAMPLER_SLOTS:
            return None
        return row.attribute

    @staticmethod
    def applicable(scene: "ShaderScene", export: "ExportingHelper | None" = None, turbo: bool = True) -> bool:
        return Sequence.taken(scene, export, turbo) is not None

    def __init__(self, scene: "ShaderScene"):
        self.scene = scene
        self.clock = ClockLoop(scene)                                  # one between the parts: the pass and matrix tables, the chunk size
        found, kinds = sources(scene)
        self.row = ROWS[kinds]
        self.attribute = self.row.attribute                            # where ShaderScene.main keeps the run
        self.piano = PianoSequence(scene) if found["piano"] else None
        self.tape = TapeSequence(scene) if found["tape"] else None
        self.video = VideoSequence(scene, self.clock) if found["video"] else None
        super().__init__([part for part in (self.piano, self.tape, self.video) if part is not None], end=self.row.end, chunked=self.row.chunked)
        self.frames = 0                                                # frames drawn by the native sequence (tests, measurements)

    def run(self, export: "ExportingHelper", turbo: bool):
        result = self.clock.run_source(export, self, turbo)
        if self.video is not None:
            self.video.raise_undecoded()                               # (a damaged Motion-JPEG frame found behind the last chunk)
        return result

    def attach(self, sequence) -> None:
        super().attach(sequence)
        if self.video is not None and len(self.parts) > 1:
            sequence.video_join = 1                                    # the video stands beside the tape or the piano on purpose (include/shaderflow_hip.h)

    def settle(self, done: int) -> None:
        self.frames = done
        super().settle(done)
