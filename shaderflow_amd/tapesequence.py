"""
TapeSequence: the frame loop of audio-reactive layered, temporal and multi-program scenes without python logic (no reference equivalent).

Three loops each stopped where the others began: `FrameTape` (tape.py) takes audio scenes of one program with one layer and no history,
`ClockLoop` (clockloop.py) takes layered / temporal / multi-program scenes in which nothing but the clock moves, `TapeLoop`
(tapeloop.py) takes audio scenes with python logic of one program. A trails or motion-blur fragment that reads `iSpectrogram`, a
two-layer multipass driven by the volume, a child program that draws the spectrum for the main one to composite: those fell through
all three into `ShaderScene.next`, which paid a device STFT, a host round trip, numpy DynamicNumber steps of every bin, the texture
writes of the spectrogram and the waveform, and the pipeline walk, every frame.

Here the device builds the audio state of a batch of frames exactly as an export's `FrameTape.build` does, and ClockLoop's native
sequence draws the batch in chunks (`sfx_sequence_run` with the tape named, by this class as its `FrameSource`): the same passes, clock ticks, rolled sampler tables, resolve
and read-out as without a tape, except that a pass whose program reads audio (samples iSpectrogram / iWaveform, or reads iAudioVolume,
iAudioVolumeIntegral, iAudioSTD, iSpectrogramOffset) takes frame k's audio state from tape frame k — a layered pass draws every layer
into row 0 of its matrix, a fused one renders into iFinal through `sfx_render_tape`. Passes that read no audio are drawn as by
ClockLoop. The next batch's build is queued right behind the last chunk of the current one and runs beside its draws.

A scene takes this loop when `main(batch=None)` finds neither FrameTape nor ClockLoop applicable (before TapeLoop) and
`SHADERFLOW_TAPE_SEQUENCE` is not "0". Out of scope, so they keep their loop: python `update()` logic (TapeLoop for one program, the frame
loop otherwise), sharded runs, a main camera away from the identity pose (`TapeLoop.camera_at_identity` says why), several audio clips
or spectrograms, and several frames per launch.
"""
from __future__ import annotations

from typing import TYPE_CHECKING

import numpy as np

from shaderflow_amd import _native as N
from shaderflow_amd.audio.module import ShaderAudio
from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
from shaderflow_amd.audio.waveform import ShaderWaveform
from shaderflow_amd.clockloop import ClockLoop, FrameSource, sequence_gate
from shaderflow_amd.parallel import shard_batches
from shaderflow_amd.tape import FrameTape
from shaderflow_amd.tapeloop import TapeLoop

if TYPE_CHECKING:
    from shaderflow_amd.exporting import ExportingHelper
    from shaderflow_amd.scene import ShaderScene


class TapeSequence(FrameSource):
    end = "last_dt"                                                    # the clock of the last frame, as FrameTape.export leaves it
    chunked = False                                                    # (a relay or SHADERFLOW_CLOCK_SEQUENCE=0: frame by frame, read out by export.pipe)

    @staticmethod
    def applicable(scene: "ShaderScene", export: "ExportingHelper | None" = None, turbo: bool = True) -> bool:
        # the audio modules of exact stock types (a subclass may update() differently from what the tape computes), and the two loudness
        # systems they own: the tape computes them; everything else must be what ClockLoop takes
        audios = [m for m in scene.modules if type(m) is ShaderAudio]
        spectrograms = [m for m in scene.modules if type(m) is ShaderSpectrogram]
        waveforms = [m for m in scene.modules if type(m) is ShaderWaveform]
        taped = (*audios, *spectrograms, *waveforms, *(s for a in audios for s in (a.volume, a.std)))
        if not audios or sequence_gate(scene, "TAPE_SEQUENCE", taped=lambda _: taped, chunked=False) is None:
            return False
        return FrameTape.audio_fits(audios, spectrograms, waveforms) and TapeSequence.camera_at_identity(scene)

    @staticmethod
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

    def __init__(self, scene: "ShaderScene"):
        self.scene = scene
        self.clock = ClockLoop(scene)                                  # the pass and matrix tables, the chunk size
        self.tape = FrameTape(scene)
        self.frames = 0                                                # frames drawn from the tape (tests, measurements)

    def run(self, export: "ExportingHelper", turbo: bool):
        return self.clock.run_source(export, self, turbo)

    # the frame source: the frames go in the tape's batches, each built (on the tape's stream, beside the previous batch's draws) and then
    # drawn in chunks. Behind the run the audio modules' host state and textures are as the export found them (FrameTape.export)

    def prepare(self, times, dts, total: int) -> None:
        tape = self.tape
        tape.prepare(total)
        if tape.spectrogram is not None and not tape.private_spectrogram:
            tape.spectrogram.configure_texture()                      # what its first update() would do (FrameTape.bind_static_uniforms)
        N.check(N.lib().sfx_tape_reset(tape.handle))

    def batches(self, total: int):
        return shard_batches(0, total, self.tape.batch)

    def begin_batch(self, first: int, size: int) -> None:
        self.tape.build(first, size)

    def attach(self, sequence) -> None:
        sequence.tape = self.tape.handle

    def take(self, sequence, first: int, count: int, batch_first: int) -> int:
        sequence.tape_frame0 = first - batch_first
        return count

    def settle(self, done: int) -> None:
        self.frames = done

    def release(self) -> None:
        self.tape.release()
