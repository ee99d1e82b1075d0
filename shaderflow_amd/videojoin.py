"""
VideoJoinedSequence: the frame loop of video scenes WITH audio modules, a piano, or both, without python logic (no reference equivalent).

A clip with its sound track — the video as background, bars, a spectrum strip or a glow from `ShaderAudio` / `ShaderSpectrogram` on top
— is the scene people write first with a `ShaderVideo`, and it fell through every sequence: the video sequence refuses the audio modules
and the piano, the tape and piano sequences refuse the video. A single-program scene of this kind went to the tape loop (tapeloop.py),
to which the video is python logic: `ShaderVideo.update()` on the host for every source frame — a flipped host copy, a synchronous
upload — and one launch per frame, nothing overlapping. A layered, temporal or multi-program one went to `ShaderScene.next` and paid the
per-frame device STFT with its host round trip and the numpy `DynamicNumber` steps as well. A piano roll over a clip: the same.

All three halves exist: `VideoSequence` (videosequence.py) stages source frames ahead of the draws and puts `k_video_frame` in front of
the frames they land on, `TapeSequence` (tapesequence.py) builds the audio state in batches and lets the passes that read audio draw
from it, `PianoSequence` (pianosequence.py) puts `k_piano_frame` and the note range in front of every frame's passes. This loop is them
as the parts of one `JoinedSource` (clockloop.py) behind one `ClockLoop`: one `sfx_sequence_run` per chunk names the video AND the tape
and / or the piano, with `video_join` set (the native call refuses the combination to a caller that does not say so). Nothing is
computed here that one of the parts does not compute on its own.

The order of the parts is piano, tape, video. The video goes last because its `take` is the one that shortens a call — to the frames
whose source frames are staged already — and what the parts in front of it set for the call does not depend on the count: the tape
sets `tape_frame0`, where the call starts inside the batch, and the piano the address of the first frame's tick. The tape is the part
that cuts the run into batches; the video shortens calls inside a batch, never across one.

What the loop itself decides: the clock behind the run is `"next"` — the video's and the piano's host state are promised to be the
frame loop's, and that is what `scene.next` leaves — and the run is `chunked` (a turbo export without a progress relay, every program
compiled), as the video sequence is. The audio modules' host state and textures stay what the export found, as under `TapeSequence`.
Behind a run, however it ended, every part settles its own: `_read`, `_exhausted`, the host copies and the frames put back in front of
the source are `VideoSequence.settle`'s, the piano's state `PianoSequence.settle`'s; a reader that failed raises its exception out of
the export once the frames staged before it are drawn, and the tape is released like every other part.

A scene takes this loop when `main(batch=None)` finds it applicable (after VideoSequence, before PianoSequence; every sequence asked
before or after refuses such a scene, the tape loop — which used to draw the single-program ones — is asked later) and none of
`SHADERFLOW_VIDEO_JOIN`, `SHADERFLOW_VIDEO_SEQUENCE` and, as they apply, `SHADERFLOW_TAPE_SEQUENCE` / `SHADERFLOW_PIANO_SEQUENCE` is
"0" — who switched a half off for an A/B run gets the host's half. Out of scope, so they keep the loop they had: everything a half
refuses (python `update()` logic, a subclassed module, several videos or pianos, `layers != 1` on the video, audio a tape does not
compute, a main camera off the identity pose beside audio, sharded runs).
"""
from __future__ import annotations

import os
from typing import TYPE_CHECKING

from shaderflow_amd.audio.module import ShaderAudio
from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
from shaderflow_amd.audio.waveform import ShaderWaveform
from shaderflow_amd.clockloop import JoinedSource, sequence_gate
from shaderflow_amd.glsl2hip import FIXED_SAMPLER_SLOTS
from shaderflow_amd.piano.module import ShaderPiano
from shaderflow_amd.pianosequence import PianoSequence, piano_fits, piano_textures
from shaderflow_amd.tape import FrameTape
from shaderflow_amd.tapesequence import TapeSequence
from shaderflow_amd.video import ShaderVideo
from shaderflow_amd.videosequence import VideoSequence, video_fits

if TYPE_CHECKING:
    from shaderflow_amd.exporting import ExportingHelper
    from shaderflow_amd.scene import ShaderScene


class VideoJoinedSequence(JoinedSource):
    @staticmethod
    def applicable(scene: "ShaderScene", export: "ExportingHelper | None" = None, turbo: bool = True) -> bool:
        # the modules of exact stock types, as the halves name them: a subclass of one, or a second piano, is left to ClockLoop's
        # judgement, which refuses it
        pianos = [m for m in scene.modules if type(m) is ShaderPiano]
        audios = [m for m in scene.modules if type(m) is ShaderAudio]
        spectrograms = [m for m in scene.modules if type(m) is ShaderSpectrogram]
        waveforms = [m for m in scene.modules if type(m) is ShaderWaveform]
        if len(pianos) > 1 or not (pianos or audios):
            return False                                               # (a video alone is VideoSequence's)
        halves = ("VIDEO_SEQUENCE", *(("PIANO_SEQUENCE",) if pianos else ()), *(("TAPE_SEQUENCE",) if audios else ()))
        if any(os.environ.get(f"SHADERFLOW_{flag}", "1") == "0" for flag in halves):
            return False
        taped = (*(t for piano in pianos for t in piano_textures(piano)), *audios, *spectrograms, *waveforms, *(s for a in audios for s in (a.volume, a.std)))
        video = sequence_gate(scene, "VIDEO_JOIN", export, turbo, ShaderVideo, taped=lambda video: (video, video.texture, *taped))
        if video is None or not video_fits(video):
            return False
        if pianos and not piano_fits(pianos[0]):
            return False
        if audios and not (FrameTape.audio_fits(audios, spectrograms, waveforms) and TapeSequence.camera_at_identity(scene)):
            return False
        # a video that goes by one of the two sampler names the tape replaces per frame would lose its slot to the tape (the native
        # call refuses such a descriptor)
        return not (audios and video.name in FIXED_SAMPLER_SLOTS)

    def __init__(self, scene: "ShaderScene"):
        self.scene = scene
        self.video = VideoSequence(scene)
        self.piano = PianoSequence(scene) if any(type(m) is ShaderPiano for m in scene.modules) else None
        self.tape = TapeSequence(scene) if any(type(m) is ShaderAudio for m in scene.modules) else None
        self.clock = self.video.clock                                  # one ClockLoop between them: the pass and matrix tables, the chunk size
        parts = [part for part in (self.piano, self.tape) if part is not None]
        if not parts:
            raise ValueError("a video without audio modules or a piano beside it is VideoSequence's")
        for part in parts:
            part.clock = self.clock
        # the video last: its `take` shortens a call; the tape is the part that cuts the run
        super().__init__((*parts, self.video), end="next", chunked=True)
        self.frames = 0                                                # frames drawn by the native sequence (tests, measurements)

    def run(self, export: "ExportingHelper", turbo: bool):
        result = self.clock.run_source(export, self, turbo)
        self.video.raise_undecoded()                                   # (a damaged Motion-JPEG frame found behind the last chunk)
        return result

    def attach(self, sequence) -> None:
        super().attach(sequence)
        sequence.video_join = 1                                        # the video stands beside the tape or the piano on purpose (include/shaderflow_hip.h)

    def settle(self, done: int) -> None:
        self.frames = done
        super().settle(done)
