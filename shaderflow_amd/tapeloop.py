"""
TapeLoop: the frame loop of audio scenes with python logic of their own, fed by the device audio tape (no reference equivalent).

`FrameTape` (tape.py) takes a scene only when nothing in it runs python between frames. A scene that overrides `update()` or
`pipeline()`, or adds a `ShaderDynamics`, a camera it moves, a texture it rewrites or a `ShaderModule` of its own — what the reference
expects users to write (shaderflow/module.py:55-116) — took the frame loop (`ShaderScene.next`), where every frame did a device STFT,
a host round trip, the numpy DynamicNumber steps of every bin and the texture writes of the spectrogram and the waveform.

User code does not change the audio of frame k unless it writes to the audio modules. So here the device still builds the audio
state of a batch of frames exactly as an export's `FrameTape.build` does (STFT, filterbank, the DynamicNumber scans, the waveform rows),
with one addition: a per-frame snapshot of every DynamicNumber's whole state (`sfx_tape_snapshot`, read back once per batch into pinned
memory). Then, frame by frame, the modules update in the frame loop's order (scene.py:456-479), except that the `update()` of each
audio module is replaced, at its own place in that order, by a *mirror step*: it sets what that `update()` would have left on the
host — `audio.tell` (the chunk reader itself still runs), the full state of `audio.volume`, `audio.std` and `spectrogram.dynamics`
(value, target, previous, derivative, acceleration, integral) and `spectrogram.offset` — to frame k's values, bit for bit. A user
module placed before the audio modules sees frame k-1's values, one placed after sees frame k's. The programs then push their
uniforms as usual and the frame is rendered from its tape slot by the fused kernel (`sfx_render_tape`), one launch per frame; the
spectrogram and waveform samplers read the tape, not their host textures.

Invalidation: before each mirror step and after each frame's updates, what the mirror set last and the tape's inputs (the dynamics
parameters, the spectrogram and waveform configuration, `speed`, `fps`) are compared with what is there. If user code wrote any of it, the
loop switches to the ordinary module updates from that point on — the host state is exact at that point, the spectrogram and
waveform textures are written once with the state they would hold — and nothing already emitted changes.

Texture writes (`ShaderTexture.write`) are ordered on the render stream behind the frames launched before them, so they need no
flush. `scene.screenshot()` during the loop returns the last frame rendered, as the frame loop would. A main camera away from the identity
pose switches to the frame loop at the first frame it is seen (`camera_at_identity` says why).

A scene takes this loop when `main(batch=None)` finds neither FrameTape nor ClockLoop applicable and `SHADERFLOW_TAPE_LOOP` is not
"0". Out of scope, so they keep the frame loop: more than one ShaderProgram, a main texture with temporal or layers != 1, subclasses of
the audio modules, an overridden `next()` or `handle()`, scheduled tasks of the scene's own, sharded and non-freewheel runs, mono clips,
an integrating spectrogram and `real` loudness systems (`applicable` says why). Rendering runs of consecutive frames with per-frame
`user[]` uniforms in one launch is a separate change: here every frame is one launch. Layered, temporal and multi-program audio scenes
WITHOUT python logic take `TapeSequence` (tapesequence.py) before this loop is asked.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import TYPE_CHECKING, Optional

import numpy as np

from shaderflow_amd import _native as N
from shaderflow_amd.audio.module import AudioMode, ShaderAudio
from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
from shaderflow_amd.audio.waveform import ShaderWaveform
from shaderflow_amd.parallel import is_sharded
from shaderflow_amd.shader import ShaderProgram
from shaderflow_amd.tape import FrameTape

if TYPE_CHECKING:
    from shaderflow_amd.exporting import ExportingHelper
    from shaderflow_amd.scene import ShaderScene

_FIELDS = ("value", "target", "previous", "derivative", "acceleration", "integral")
_PARAMETERS = ("frequency", "zeta", "response", "precision", "integrate")


def _dynamics_state(system) -> tuple:
    """Everything of a DynamicNumber that the tape either sets or was built from, as comparable bytes"""
    out = []
    for name in _FIELDS:
        value = np.asarray(getattr(system, name))
        out.append((value.dtype.str, value.shape, value.tobytes()))
    return (*out, *(getattr(system, name) for name in _PARAMETERS))


class TapeLoop:
    attribute = "tape_loop"                                            # where ShaderScene.main keeps the loop that ran

    @staticmethod
    def applicable(scene: "ShaderScene", export: "ExportingHelper | None" = None, turbo: bool = True) -> bool:
        from shaderflow_amd.scene import ShaderScene
        if os.environ.get("SHADERFLOW_TAPE_LOOP", "1") == "0":
            return False
        if not scene.freewheel or is_sharded():
            return False
        if type(scene).next is not ShaderScene.next or type(scene).handle is not ShaderScene.handle:
            return False
        if any(task is not scene.vsync for task in scene.scheduler.tasks):
            return False
        audios, spectrograms, waveforms = [], [], []
        for module in scene.modules:
            if module is scene:
                continue
            if isinstance(module, ShaderProgram) and module not in (scene.shader, scene._final):
                return False
            if isinstance(module, (ShaderAudio, ShaderSpectrogram, ShaderWaveform)):
                if type(module) not in (ShaderAudio, ShaderSpectrogram, ShaderWaveform):
                    return False                                  # a subclass may update() differently from what the tape computes
                {ShaderAudio: audios, ShaderSpectrogram: spectrograms, ShaderWaveform: waveforms}[type(module)].append(module)
        if scene.shader.texture.temporal != 1 or scene.shader.texture.layers != 1:
            return False
        if not audios or not FrameTape.audio_fits(audios, spectrograms, waveforms):
            return False
        audio = audios[0]
        # two limits beyond the tape's own, because the mirror must reproduce the host objects and not only what the render reads:
        # ShaderSpectrogram.update reshapes its targets to TWO rows (spectrogram.py:306), so a mono clip's host state is not the tape's
        # (channels, bins) state; and the scan never integrates the bins (the render does not read their integral), so an integrating
        # spectrogram's `integral` could not be mirrored. `real` loudness systems step with rdt, the tape's coefficients come from dt.
        if audio.channels != 2 or audio.mode != AudioMode.File:
            return False
        if spectrograms and spectrograms[0].dynamics.integrate:
            return False
        if audio.volume.real or audio.std.real:
            return False
        return True

    def __init__(self, scene: "ShaderScene"):
        self.scene = scene
        self.tape = FrameTape(scene)
        tape = self.tape
        self.audio: ShaderAudio = tape.audio
        self.spectrogram: Optional[ShaderSpectrogram] = None if tape.private_spectrogram else tape.spectrogram
        self.waveform: Optional[ShaderWaveform] = tape.waveform
        self.programs = [m for m in reversed(scene.modules) if isinstance(m, ShaderProgram)]
        # the module → mirror step map, in the scene's module order
        self.mirrors = {id(self.audio): self.mirror_audio, id(self.audio.volume): self.mirror_volume, id(self.audio.std): self.mirror_std}
        if self.spectrogram is not None:
            self.mirrors[id(self.spectrogram)] = self.mirror_spectrogram
        if self.waveform is not None:
            self.mirrors[id(self.waveform)] = self.mirror_waveform
        self.expected: dict = {}                                  # id(module) → its state as the last mirror step left it
        self.live = True
        self.frames_mirrored = 0                                  # frames rendered from the tape (tests, measurements)
        self.wave_tell: Optional[int] = None                      # `tell` the waveform texture would have been written at

    # what the tape was built from, and what each mirror step sets ---------------------------------------------------------------

    def fingerprint(self, module) -> tuple:
        audio = self.audio
        if module is audio:
            return (audio.tell, audio.native.value if audio.native is not None else None, audio.samplerate, audio.channels, self.scene.speed)
        if module is audio.volume or module is audio.std:
            return (*_dynamics_state(module), module.real)
        if module is self.spectrogram:
            spec = module
            return (spec.offset, hash(spec), spec.window, spec.length_samples, spec.audio is audio, spec.device_magnitude,
                    _dynamics_state(spec.dynamics))
        if module is self.waveform:
            wave = module
            return (wave.length, wave.samplerate, wave.reducer, wave._points, wave.chunk_size, wave.audio is audio)
        raise KeyError(module)

    def dirty(self, module) -> bool:
        expected = self.expected.get(id(module))
        return expected is not None and expected != self.fingerprint(module)

    # mirror steps: frame k's values from the snapshot (slot j of the batch) --------------------------------------------------------

    def mirror_audio(self, j: int) -> None:
        audio = self.audio
        try:                                                      # the chunk reader runs as in ShaderAudio.update: `data` stays the history
            if audio._file_stream:
                audio._file_reader.chunk = self.scene.rdt
                audio.add_data(next(audio._file_stream).T)
        except StopIteration:
            pass
        if audio.tell != self.tell[self.first + j]:
            raise RuntimeError(f"TapeLoop: audio.tell {audio.tell} disagrees with the tape's schedule {self.tell[self.first + j]}")
        audio.volume.target = np.float32(self.state64[j, 0, 1])
        audio.std.target = np.float32(self.state64[j, 1, 1])
        for system in (audio.volume, audio.std):                  # (what this step set is not a user's write)
            self.expected[id(system)] = self.fingerprint(system)

    def _mirror_scalar(self, system, row) -> None:
        # what DynamicNumber.next leaves (dynamics.py:197-250): a step replaces `previous` by the target object and `acceleration` by a
        # float64 scalar, and updates value / derivative / integral in place
        dt = abs(self.scene.dt)
        stepped = bool(dt) and not (np.abs(system.target - system.value).max() < system.precision)
        system.value[...] = row[0]
        if stepped:
            system.previous = system.target
            system.acceleration = np.float64(row[4])
        np.asarray(system.derivative)[...] = row[3]
        if system.integrate and dt:
            np.asarray(system.integral)[...] = row[5]

    def mirror_volume(self, j: int) -> None:
        self._mirror_scalar(self.audio.volume, self.state64[j, 0])

    def mirror_std(self, j: int) -> None:
        self._mirror_scalar(self.audio.std, self.state64[j, 1])

    def mirror_spectrogram(self, j: int) -> None:
        spec = self.spectrogram
        spec.configure_texture()
        spec.offset = (spec.offset + 1) % spec.length_samples
        dyn, shape = spec.dynamics, spec._row_shape
        if dyn.value.shape != shape:
            dyn.set(np.zeros(shape, dtype=np.float32))
        row = self.state32[j]
        dyn.target = row[1].reshape(shape).copy()
        stepped = bool(self.scene.dt) and not (np.abs(dyn.target - dyn.value).max() < dyn.precision)
        dyn.value[...] = row[0].reshape(shape)
        if stepped:
            dyn.previous = dyn.target
            dyn.derivative[...] = row[3].reshape(shape)
            dyn.acceleration = row[4].reshape(shape).copy()
        self.columns[:, spec.offset, :] = row[0].reshape(spec.spectrogram_bins, self.audio.channels)

    def mirror_waveform(self, j: int) -> None:
        wave = self.waveform
        if wave.texture.components != self.audio.channels:
            wave.texture.components = self.audio.channels
        self.wave_tell = self.audio.tell

    # the switch to the ordinary updates -------------------------------------------------------------------------------------------

    def switch(self, export: "ExportingHelper") -> None:
        """The current frame, from the module being updated on, and every frame after it take the ordinary module updates"""
        scene = self.scene
        self.live = False
        export.drain()
        if self.last_frame is not None:
            scene.write_final(self.last_frame, self.top_down)    # iFinal holds the previous frame, as in the frame loop
        scene.__dict__.pop("screenshot", None)
        # the textures the mirror did not write: as the last mirrored update() would have left them
        if self.spectrogram is not None and self.expected.get(id(self.spectrogram)) is not None:
            self.spectrogram.texture.write(np.ascontiguousarray(self.columns))
        if self.waveform is not None and self.wave_tell is not None:
            self.waveform.texture.write(self.waveform.rows([self.wave_tell])[0])

    # the loop ---------------------------------------------------------------------------------------------------------------------

    def read_state(self, count: int) -> None:
        n = self.values
        raw = np.empty(count*(96 + 24*n), np.uint8)
        N.check(N.lib().sfx_tape_read(self.tape.handle, N.TAPE_STATE, 0, count, raw.ctypes.data, raw.nbytes))
        self.state64 = raw[:count*96].view(np.float64).reshape(count, 2, 6)
        self.state32 = raw[count*96:].view(np.float32).reshape(count, 6, n)

    def frame_updates(self, j: int, export: "ExportingHelper") -> None:
        """Every module's update of the frame in tape slot j, in the frame loop's order, audio modules mirrored while the tape holds"""
        for module in self.scene.modules:
            if isinstance(module, ShaderProgram):
                continue
            if self.live:
                step = self.mirrors.get(id(module))
                if step is not None:
                    # (the audio step sets the loudness targets: the two systems must be as the mirror left them before it)
                    shared = (self.audio.volume, self.audio.std) if module is self.audio else ()
                    if self.dirty(module) or any(self.dirty(system) for system in shared) or self.inputs_changed():
                        self.switch(export)
                    else:
                        step(j)
                        self.expected[id(module)] = self.fingerprint(module)
                        continue
            module.update()

    def inputs_changed(self) -> bool:
        return self.scene.speed != self.speed or self.scene.fps != self.fps

    def run(self, export: "ExportingHelper", turbo: bool):
        from shaderflow_amd.parallel import shard_batches
        from shaderflow_amd.scheduler import freewheel_clock
        scene, tape, context = self.scene, self.tape, self.scene.context
        total = export.total_frames
        self.speed, self.fps, self.top_down = scene.speed, scene.fps, export.top_down
        _, _, rdts = freewheel_clock(scene.fps, total, scene.speed)
        tape.prepare(total)
        self.tell = tape.tell
        N.check(N.lib().sfx_tape_snapshot(tape.handle, 1))
        tape.bind_static_uniforms()
        N.check(N.lib().sfx_tape_reset(tape.handle))
        self.values = tape.spectrogram.spectrogram_bins*self.audio.channels
        if self.spectrogram is not None:
            self.columns = np.zeros((self.spectrogram.spectrogram_bins, self.spectrogram.length_samples, self.audio.channels), np.float32)
        frame_bytes = scene.width*scene.height*3
        batches = shard_batches(0, total, tape.batch)
        buffers = [context.alloc(frame_bytes*tape.batch) for _ in range(2)]
        self.last_frame: Optional[int] = None
        original_screenshot = scene.screenshot

        def screenshot() -> np.ndarray:                          # the last frame rendered, through iFinal as in the frame loop
            if self.last_frame is not None:
                scene.write_final(self.last_frame, self.top_down)
            return original_screenshot()
        scene.screenshot = screenshot
        shader, ssaa_x1000 = scene.shader, int(round(scene.ssaa*1000))
        time, dt = 0.0, 0.0
        self.camera_seen, self.camera_identity = None, True
        try:
            tape.build(*batches[0])
            self.read_state(batches[0][1])
            for index, (first, count) in enumerate(batches):
                buffer = buffers[index % 2]
                self.first = first
                export.render_waits_for_last_read()               # this buffer's frames of two batches ago have left it
                for j in range(count):
                    k = first + j
                    if scene.quit:                                # ShaderMessage.Window.Close, as the vsync loop honours it
                        break
                    # what scene.next integrated after frame k-1 (scene.py:475-479): the freewheel clock's operations (scheduler.py)
                    dt = rdts[k]*scene.speed
                    time += dt
                    scene.time, scene.dt, scene.rdt = time, dt, rdts[k]
                    scene._fused_this_frame = False
                    self.frame_updates(j, export)
                    if self.live and (self.inputs_changed() or any(self.dirty(m) for m in self.mirrored())):
                        self.switch(export)
                    if self.live:
                        shader.use_scene_pipeline()
                        if not self.camera_at_identity():
                            self.switch(export)
                    if self.live:
                        target = buffer + j*frame_bytes
                        N.check(N.lib().sfx_render_tape(shader.program, tape.handle, j, 1, scene.width, scene.height, ssaa_x1000,
                                                        scene.subsample, C.c_void_p(target)))
                        self.last_frame = target
                        self.frames_mirrored += 1
                        # read out frame by frame, as the frame loop does: the host's python of the next frames overlaps the copy
                        export.pipe_device(target, rgb=True, turbo=turbo)
                        export.update()
                    else:
                        for program in self.programs:
                            program.update()
                        export.pipe(turbo=turbo)
                        export.update()
                if scene.quit:
                    break
                if self.live and index + 1 < len(batches):
                    tape.build(*batches[index + 1])               # on the tape's stream, beside this batch's renders
                    self.read_state(batches[index + 1][1])
            if self.live and self.last_frame is not None:
                scene.write_final(self.last_frame, self.top_down)  # iFinal holds the last frame, as the frame loop leaves it
            return export.finish()                              # (the scene's clock stays that of the last frame, as in FrameTape)
        finally:
            scene.__dict__.pop("screenshot", None)
            context.synchronize()
            export.drain()
            for pointer in buffers:
                context.free(pointer)
            tape.release()

    # glsl.hpp camera_is_identity(): the pose under which the launch of a tape frame and of a frame-loop frame pick the same kernels
    IDENTITY = {"iCameraProjection": (np.int32, (0,)), "iCameraPosition": (np.float32, (0, 0, 0)), "iCameraRight": (np.float32, (1, 0, 0)),
                "iCameraUpward": (np.float32, (0, 1, 0)), "iCameraForward": (np.float32, (0, 0, 1)), "iCameraZoom": (np.float32, (1,)),
                "iCameraIsometric": (np.float32, (0,)), "iCameraFocalLength": (np.float32, (1,)), "iCameraOrbital": (np.float32, (0,)),
                "iCameraDolly": (np.float32, (0,))}

    def camera_at_identity(self) -> bool:
        """Whether the main program's camera uniforms, as last sent, are the identity camera's (compared as numbers, like the library).
        Any other pose takes the frame loop: sfx_render_tape bounds the visualizer kernels' texel windows without the frame's blur
        intensity (it lives on the device), sfx_render_resolve with it, so the two launches may pick different block and tile
        configurations — and under a non-identity camera those configurations differ by 1 LSB on some frames (the pixel tier and the
        tiled kernels alike). Under the identity camera they agree to the bit."""
        pushed = self.scene.shader._pushed
        seen = tuple(pushed[name][0] if name in pushed else None for name in self.IDENTITY)
        if seen != self.camera_seen:
            self.camera_seen = seen
            self.camera_identity = all(raw is None or np.array_equal(np.frombuffer(raw[1], dtype)[:len(want)], want)
                                       for raw, (dtype, want) in zip(seen, self.IDENTITY.values()))
        return self.camera_identity

    def mirrored(self):
        for module in self.scene.modules:
            if id(module) in self.mirrors:
                yield module
