"""
PianoTapeSequence: the frame loop of piano-roll scenes WITH their sound track, without python logic (no reference equivalent).

A piano roll and the audio that plays it — keys and falling notes from a `ShaderPiano`, a spectrum strip or a glow from `ShaderAudio` /
`ShaderSpectrogram` — is the scene users write first, and it fell through every fast loop: the tape loops refuse the piano, the piano
sequence refuses the audio modules. `ShaderScene.next` then paid, per frame, `ShaderPiano.update()` with its 512 KB upload, a device
STFT with a host round trip, numpy `DynamicNumber` steps of every bin, and the pipeline walk.

Both halves exist: `PianoSequence` (pianosequence.py) puts `k_piano_frame` and the note range in front of every frame's passes,
`TapeSequence` (tapesequence.py) builds the audio state in batches and lets the passes that read audio draw from it. This loop is the
two of them as the parts of one `JoinedSource` (clockloop.py) behind one `ClockLoop`: one `sfx_sequence_run` per chunk names the tape
AND the piano. Nothing is computed here that one of the parts does not compute on its own.

What the loop itself decides: the clock behind the run is `"next"` — the piano's host state is promised to be the frame loop's, and that
is what `scene.next` leaves — and the run is `chunked` (a turbo export without a progress relay, every program compiled), as the piano
sequence is. The audio modules' host state and textures stay what the export found, as under `TapeSequence`.

A scene takes this loop when `main(batch=None)` finds it applicable (after PianoSequence, before TapeSequence; both refuse such a scene)
and none of `SHADERFLOW_PIANO_TAPE`, `SHADERFLOW_PIANO_SEQUENCE`, `SHADERFLOW_TAPE_SEQUENCE` is "0" — who switched a half off for an
A/B run gets the host's half. Out of scope, so they keep the frame loop: everything either half refuses (python `update()` logic,
subclassed or several pianos, subclassed audio modules, audio a tape does not compute, a main camera off the identity pose, sharded
runs). With a video beside them the scene is `VideoJoinedSequence`'s (videojoin.py), asked before this loop.
"""
from __future__ import annotations

import os
from typing import TYPE_CHECKING

from shaderflow_amd.audio.module import ShaderAudio
from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
from shaderflow_amd.audio.waveform import ShaderWaveform
from shaderflow_amd.clockloop import JoinedSource, sequence_gate
from shaderflow_amd.piano.module import ShaderPiano
from shaderflow_amd.pianosequence import PianoSequence, piano_fits, piano_textures
from shaderflow_amd.tape import FrameTape
from shaderflow_amd.tapesequence import TapeSequence

if TYPE_CHECKING:
    from shaderflow_amd.exporting import ExportingHelper
    from shaderflow_amd.scene import ShaderScene


class PianoTapeSequence(JoinedSource):
    @staticmethod
    def applicable(scene: "ShaderScene", export: "ExportingHelper | None" = None, turbo: bool = True) -> bool:
        if any(os.environ.get(f"SHADERFLOW_{flag}", "1") == "0" for flag in ("PIANO_SEQUENCE", "TAPE_SEQUENCE")):
            return False
        # the audio modules of exact stock types and their two loudness systems, as TapeSequence.applicable names them: a subclass of one
        # is left to ClockLoop's judgement, which refuses it
        audios = [m for m in scene.modules if type(m) is ShaderAudio]
        spectrograms = [m for m in scene.modules if type(m) is ShaderSpectrogram]
        waveforms = [m for m in scene.modules if type(m) is ShaderWaveform]
        taped = (*audios, *spectrograms, *waveforms, *(s for a in audios for s in (a.volume, a.std)))
        piano = sequence_gate(scene, "PIANO_TAPE", export, turbo, ShaderPiano, taped=lambda piano: (*piano_textures(piano), *taped))
        if piano is None or not piano_fits(piano):
            return False
        if not audios or not FrameTape.audio_fits(audios, spectrograms, waveforms):
            return False
        return TapeSequence.camera_at_identity(scene)

    def __init__(self, scene: "ShaderScene"):
        self.scene = scene
        self.piano, self.tape = PianoSequence(scene), TapeSequence(scene)
        self.clock = self.piano.clock                                  # one ClockLoop between them: the pass and matrix tables, the chunk size
        self.tape.clock = self.clock
        # the piano first: the tape is the part that cuts the run, and neither shortens a call
        super().__init__((self.piano, self.tape), end="next", chunked=True)
        self.frames = 0                                                # frames drawn by the native sequence (tests, measurements)

    def run(self, export: "ExportingHelper", turbo: bool):
        return self.clock.run_source(export, self, turbo)

    def settle(self, done: int) -> None:
        self.frames = done
        super().settle(done)
