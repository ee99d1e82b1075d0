"""
TapeSequence: the audio tape in front of the frames of audio-reactive layered, temporal and multi-program scenes without python logic (no
reference equivalent).

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

Which scenes run this way, alone or beside a piano or a video, is `Sequence`'s to say (sequence.py), asked by `main(batch=None)` behind
FrameTape and ClockLoop and before TapeLoop. Out of scope, so they keep their loop: python `update()` logic (TapeLoop for one program, the
frame loop otherwise), sharded runs, a main camera away from the identity pose (`TapeLoop.camera_at_identity` says why), several audio
clips or spectrograms, and several frames per launch.
"""
from __future__ import annotations

from typing import TYPE_CHECKING

from shaderflow_amd import _native as N
from shaderflow_amd.clockloop import FrameSource
from shaderflow_amd.parallel import shard_batches
from shaderflow_amd.tape import FrameTape

if TYPE_CHECKING:
    from shaderflow_amd.scene import ShaderScene


class TapeSequence(FrameSource):
    def __init__(self, scene: "ShaderScene"):
        self.scene = scene
        self.tape = FrameTape(scene)

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

    def release(self) -> None:
        self.tape.release()
