"""
FrameTape: the batched export path (no reference equivalent; SURVEY.md §7 "Tape, not per-frame host round-trips").

In an export the whole audio file and the frame clock are known up front, so nothing the modules compute between
two frames needs python: for a batch of frames the device computes the STFT of every frame, the filterbank
product, the DynamicNumber recurrences (spectrogram bins in float32, volume/std in float64), the waveform rows
and the per-frame uniforms, keeps them in HBM, and the fused fragment kernel renders the batch back to back
(`sfx_tape_build` + `sfx_render_tape`). The host contributes exactly what the reference evaluates in python
scalars: the scheduler's float64 clock, the PCM chunk schedule, and the per-frame DynamicNumber coefficients
(branch selection, exp/cos — dynamics.py:231-242), rounded to float32 where numpy would round them.

A scene qualifies when it is made only of the stock modules and nothing overrides `update()`/`pipeline()`;
anything else runs through the frame loop (`ShaderScene.next`), which produces the same frames. Out of scope here: a main texture
with `temporal` or `layers` != 1 and programs besides the main one and `_final` — audio scenes of that kind without python logic take
`TapeSequence` (tapesequence.py: this tape, drawn by the native clock sequence), those with python logic `TapeLoop` or the frame loop.

`FrameTape.export` runs one function per delivery mode (`delivery_mode`): `export_single` (one process), `export_host` and
`export_device` (sharded over a process group, parallel.py); each renders its batches as sink frames (exporting.SinkBatches).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import TYPE_CHECKING, Optional

import numpy as np

from shaderflow_amd import _native as N
from shaderflow_amd.audio.module import ShaderAudio
from shaderflow_amd.audio.reader import chunk_schedule
from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
from shaderflow_amd.audio.waveform import ShaderWaveform, WaveformReducer
from shaderflow_amd.camera import ShaderCamera
from shaderflow_amd.dynamics import ShaderDynamics, dynamics_coefficients
from shaderflow_amd.exporting import SinkBatches
from shaderflow_amd.module import ShaderModule
from shaderflow_amd.parallel import (DeviceArray, PeerWindowsUnavailable, RangeTransfer, SdmaTransfer, contiguous_device_export, host_export,
                                     is_sharded, rank_world, shard_batches, shard_frames, shard_mode)
from shaderflow_amd.piano import PianoNote
from shaderflow_amd.scheduler import freewheel_clock
from shaderflow_amd.shader import ShaderProgram
from shaderflow_amd.texture import ShaderTexture

if TYPE_CHECKING:
    from shaderflow_amd.exporting import ExportingHelper
    from shaderflow_amd.scene import ShaderScene


def _coefficients_f64(system, dts) -> np.ndarray:
    out = np.zeros(len(dts), dtype=[("dt", "f8"), ("k1", "f8"), ("k2", "f8"), ("k3", "f8")])
    for k, dt in enumerate(dts):
        dt = abs(dt)
        if dt:
            k1, k2, k3, _ = dynamics_coefficients(system.frequency, system.zeta, system.response, dt)
            out[k] = (dt, k1, k2, k3)
    return out


def _coefficients_f32(system, dts) -> np.ndarray:
    wide = _coefficients_f64(system, dts)
    out = np.zeros(len(dts), dtype=[("dt", "f4"), ("k1", "f4"), ("k2", "f4"), ("k3", "f4")])
    for name in ("dt", "k1", "k2", "k3"):
        out[name] = wide[name].astype(np.float32)       # python scalar → float32, as numpy does for a float32 array
    return out


class FrameTape:
    BATCH = 60
    SCROLL_BYTES = 8 << 30           # per-frame states of a scrolling spectrogram texture that one batch may hold

    @staticmethod
    def applicable(scene: "ShaderScene") -> bool:
        from shaderflow_amd.scene import ShaderScene
        if type(scene).update is not ShaderModule.update or type(scene).pipeline is not ShaderScene.pipeline:
            return False
        stock = (ShaderCamera, ShaderDynamics, ShaderProgram, ShaderTexture, ShaderAudio, ShaderSpectrogram, ShaderWaveform)
        audios, spectrograms, waveforms = [], [], []
        for module in scene.modules:
            if module is scene or (hasattr(module, "__eq__") and isinstance(module, ShaderScene)):
                continue
            if type(module) not in stock:
                return False
            if isinstance(module, ShaderProgram) and module not in (scene.shader, scene._final):
                return False
            if isinstance(module, ShaderAudio):
                audios.append(module)
            elif isinstance(module, ShaderSpectrogram):
                spectrograms.append(module)
            elif isinstance(module, ShaderWaveform):
                waveforms.append(module)
        if scene.shader.texture.temporal != 1 or scene.shader.texture.layers != 1:
            return False
        if not (audios or spectrograms or waveforms):
            return True                                           # clock tape: only iTime/iTau/iFrame change between frames
        return FrameTape.audio_fits(audios, spectrograms, waveforms)

    @staticmethod
    def audio_fits(audios: list, spectrograms: list, waveforms: list) -> bool:
        """Whether these audio modules of a scene (at least one of them) are what a tape computes: one ShaderAudio with device PCM, at
        most one spectrogram and one waveform of it, a magnitude the STFT kernel evaluates, and sizes the scan and one batch hold"""
        if len(audios) != 1 or len(spectrograms) > 1 or len(waveforms) > 1:
            return False
        audio = audios[0]
        if audio.native is None or any(m.audio is not audio for m in (*spectrograms, *waveforms)):
            return False
        if not spectrograms:
            return True                                           # Waveform-like scenes: the tape carries a private spectrogram nobody samples
        if not spectrograms[0].device_magnitude:
            return False                                          # a `magnitude` callable of the user's own runs on the host, frame by frame (audio/spectrogram.py)
        if spectrograms[0].spectrogram_bins*audio.channels > 16384:
            return False                                          # the scan kernel walks up to 16 384 values per frame (csrc/capi_audio.hip DYNAMICS_SCAN_LIMIT)
        # a scrolling spectrogram (length > 0) keeps one state of its texture per frame of a batch in HBM (sfx_tape_desc.length_samples)
        if spectrograms[0].length_samples*spectrograms[0].spectrogram_bins*audio.channels*4*FrameTape.BATCH > FrameTape.SCROLL_BYTES:
            return False
        return True                                               # any (ssaa, subsample): fused when possible, else two passes

    def __init__(self, scene: "ShaderScene", batch: Optional[int] = None, use_mfma: Optional[bool] = None):
        self.scene = scene
        self.batch = int(batch or self.BATCH)
        # filterbank product: CSR rows in scipy's summation order (bit-exact against the reference's `M.dot`, the default) or the
        # dense banded GEMM on v_mfma_f32_32x32x2_f32 (2e-6 relative: another summation order); SHADERFLOW_FILTERBANK=mfma|csr
        if use_mfma is None:
            use_mfma = os.environ.get("SHADERFLOW_FILTERBANK", "csr").lower() == "mfma"
        self.use_mfma = bool(use_mfma)
        self.audio: Optional[ShaderAudio] = next((m for m in scene.modules if isinstance(m, ShaderAudio)), None)
        self.spectrogram: Optional[ShaderSpectrogram] = next((m for m in scene.modules if isinstance(m, ShaderSpectrogram)), None)
        self.waveform: Optional[ShaderWaveform] = next((m for m in scene.modules if isinstance(m, ShaderWaveform)), None)
        self.private_spectrogram = False
        if self.audio is not None and self.spectrogram is None:
            # A scene with audio but no spectrogram module (demo.py's Waveform, or a fragment that reads iAudioVolume only): the native
            # tape is built around a spectrogram plan, so it gets the smallest one — detached from the scene again, so that no sampler,
            # uniform or update() of it exists as far as the scene is concerned (20 µs of STFT per 60 frames buys the batched path)
            registered = len(scene.modules)
            self.spectrogram = ShaderSpectrogram(scene=scene, audio=self.audio, length=0, name="iTapePrivateSpectrogram")
            self.spectrogram.fft_n = 8
            self.spectrogram.from_notes(start=PianoNote.from_frequency(440.0), end=PianoNote.from_frequency(880.0), bins=2)
            del scene.modules[registered:]
            self.private_spectrogram = True
        self.handle: Optional[N.Handle] = None
        self.frames = 0

    # host-side schedule -----------------------------------------------------------------------------------------

    def prepare(self, frames: int) -> "FrameTape":
        """Everything python contributes, for `frames` frames from time 0"""
        scene, audio, spec = self.scene, self.audio, self.spectrogram
        self.frames = frames
        times, dts, rdts = freewheel_clock(scene.fps, frames, scene.speed)
        self.times, self.dts = times, dts
        self.release()
        if audio is None:                                    # clock tape (scenes without audio modules)
            self.clock = np.zeros(frames, dtype=[("iTime", "f4"), ("iTau", "f4"), ("iSpectrogramOffset", "f4"), ("iFrame", "i4")])
            for k, t in enumerate(times):
                self.clock[k] = (t, (t/scene.runtime) % 1.0, 0.0, round(t*scene.fps))
            handle = N.Handle()
            N.check(N.lib().sfx_clock_tape_create(scene.context.handle, self.batch, C.byref(handle)))
            self.handle = handle
            return self
        self.tell = chunk_schedule(rdts, int(audio.samplerate), audio.channels, audio._file_reader.samples.shape[0])
        self.clock = np.zeros(frames, dtype=[("iTime", "f4"), ("iTau", "f4"), ("iSpectrogramOffset", "f4"), ("iFrame", "i4")])
        width = spec.length_samples
        for k, t in enumerate(times):
            self.clock[k] = (t, (t/scene.runtime) % 1.0, ((k + 1) % width)/width, round(t*scene.fps))
        self.spec_coeff = _coefficients_f32(spec.dynamics, dts)
        self.vol_coeff = _coefficients_f64(audio.volume, dts)
        self.std_coeff = _coefficients_f64(audio.std, dts)

        reducer = self.waveform.reducer if self.waveform is not None else WaveformReducer.Average
        desc = N.TapeDesc(
            points=(self.waveform._points if self.waveform is not None else 0),
            chunk_size=(self.waveform.chunk_size if self.waveform is not None else 1),
            reducer=WaveformReducer(reducer).value,
            volume_window=int(0.1*audio.samplerate),
            use_mfma=int(self.use_mfma),
            volume_integrate=int(audio.volume.integrate), std_integrate=int(audio.std.integrate),
            length_samples=int(spec.length_samples),
            precision=float(spec.dynamics.precision),
        )
        handle = N.Handle()
        N.check(N.lib().sfx_tape_create(spec.plan(), audio.native, C.byref(desc), self.batch, C.byref(handle)))
        self.handle = handle
        return self

    def release(self) -> None:
        if self.handle is not None and self.handle.value:
            N.lib().sfx_tape_destroy(self.handle)
        self.handle = None

    def bind_static_uniforms(self) -> None:
        """Uniforms and samplers that do not change over the export (scene.py:687-703 etc.), pushed once"""
        program = self.scene.shader
        if program.program is None:
            program.compile()
        if self.spectrogram is not None and not self.private_spectrogram:
            self.spectrogram.configure_texture()             # what its first update() would do
        program.use_pipeline(program.full_pipeline())

    # device work --------------------------------------------------------------------------------------------------

    def build(self, first: int, count: int) -> None:
        """Audio state of frames [first, first+count) → tape slots [0, count). Frames must be visited in order."""
        s = slice(first, first + count)
        if self.audio is None:
            clock = np.ascontiguousarray(self.clock[s])
            N.check(N.lib().sfx_tape_build(self.handle, count, None, C.cast(clock.ctypes.data, C.POINTER(N.FrameClock)), None, None, None))
            return
        tell = np.ascontiguousarray(self.tell[s])
        clock, spec = np.ascontiguousarray(self.clock[s]), np.ascontiguousarray(self.spec_coeff[s])
        vol, std = np.ascontiguousarray(self.vol_coeff[s]), np.ascontiguousarray(self.std_coeff[s])
        N.check(N.lib().sfx_tape_build(self.handle, count, N.as_ptr(tell, C.c_int64),
                                       C.cast(clock.ctypes.data, C.POINTER(N.FrameClock)),
                                       C.cast(spec.ctypes.data, C.POINTER(N.DynCoeffF32)),
                                       C.cast(vol.ctypes.data, C.POINTER(N.DynCoeffF64)),
                                       C.cast(std.ctypes.data, C.POINTER(N.DynCoeffF64))))

    def render(self, count: int, device_out: int, first_slot: int = 0) -> None:
        """Tape slots [first_slot, first_slot+count) → `count` RGB8 frames at `device_out`"""
        scene = self.scene
        N.check(N.lib().sfx_render_tape(scene.shader.program, self.handle, first_slot, count, scene.width, scene.height,
                                        int(round(scene.ssaa*1000)), scene.subsample, C.c_void_p(device_out)))

    def read(self, what: int, count: int, first_slot: int = 0) -> np.ndarray:
        """Tape content for inspection (tests)"""
        if self.audio is None:
            bins, channels = 1, 1
        else:
            bins, channels = self.spectrogram.spectrogram_bins, self.audio.channels
        shapes = {
            N.TAPE_SPECTROGRAM: (count, bins, channels), N.TAPE_TARGETS: (count, bins, channels),
            N.TAPE_WAVEFORM: (count, self.waveform._points if self.waveform is not None else 1, channels),
            N.TAPE_UNIFORMS: (count, 8), N.TAPE_LOUDNESS: (count, 2),
            N.TAPE_SCROLL: (count, bins, self.spectrogram.length_samples if self.spectrogram is not None else 1, channels),
        }
        out = np.zeros(shapes[what], np.float32)
        N.check(N.lib().sfx_tape_read(self.handle, what, first_slot, count, out.ctypes.data, out.nbytes))
        return out

    # whole export ---------------------------------------------------------------------------------------------------

    def export(self, export: "ExportingHelper", turbo: bool = True):
        """The whole export: the tape of every frame, one delivery mode (`delivery_mode`) to move the finished frames to the sink, and the
        scene's clock left at the last frame's"""
        scene = self.scene
        self.prepare(export.total_frames)
        self.bind_static_uniforms()
        N.check(N.lib().sfx_tape_reset(self.handle))
        mode = self.delivery_mode(export)
        try:
            if mode == "single":
                self.export_single(export, turbo)
            elif mode == "host":
                self.export_host(export)
            else:
                self.export_device(export, mode, turbo)
            scene.time, scene.dt, scene.rdt = self.times[-1], self.dts[-1], self.dts[-1]      # clock of the last frame
            return export.finish()
        finally:
            scene.context.synchronize()
            self.release()

    def delivery_mode(self, export: "ExportingHelper") -> str:
        """"single" without a sharded process group, else SHADERFLOW_SHARD's mode. The device modes keep every frame of the export resident
        in rank 0's HBM (a 60 s 4K clip: 89.6 GB of 288): a clip that does not fit falls back to host mode — for ALL ranks: rank 0
        decides, everybody follows"""
        if not is_sharded():
            return "single"
        mode = shard_mode()
        if not mode.startswith("device"):
            return mode
        import torch
        import torch.distributed as dist
        rank, total = rank_world()[0], export.total_frames
        verdict = [True]
        if rank == 0:
            verdict[0] = total*export.frame_bytes + (4 << 30) < torch.cuda.mem_get_info(self.scene.context.device)[0]
        dist.broadcast_object_list(verdict, src=0)
        if verdict[0]:
            return mode
        if rank == 0:
            print(f"shaderflow_amd: {total} frames of {export.frame_bytes >> 20} MiB do not fit rank 0's free device memory: "
                  f"SHADERFLOW_SHARD={mode} falls back to host mode", flush=True)
        return "host"

    def export_single(self, export: "ExportingHelper", turbo: bool) -> None:
        """One process: a software pipeline over two batch buffers — batch b+1 renders while the frames of batch b travel to the host"""
        batches = shard_batches(0, export.total_frames, self.batch)
        sink = SinkBatches(export, self.batch)

        def render(index: int) -> None:
            first, count = batches[index]
            self.build(first, count)
            sink.render(sink.buffers[index % 2], count, self.render)
            export.fence(index % 2)
        try:
            render(0)
            for index, (_, count) in enumerate(batches):
                if index + 1 < len(batches):
                    export.render_waits_for_last_read()          # buffers[(index+1) % 2] held batch index-1
                    render(index + 1)
                export.pipe_device_frames(sink.buffers[index % 2], export.frame_bytes, count, turbo=turbo, fence=index % 2)
            # leave the last frame in iFinal, where the frame loop would have left it (scene.screenshot())
            self.scene.write_final(sink.last_rgb, export.top_down)
        finally:
            sink.close()

    def export_host(self, export: "ExportingHelper") -> None:
        """Every rank reads its own batches out into shared memory, rank 0's writer thread hands them to the sink in frame order
        (parallel.host_export). The ring holds a batch and a few frames per rank: room for the batch a rank produces while its previous
        one is being taken (two batches per rank asked /dev/shm for 24 GB at 8 ranks of 4K)"""
        rank, world = rank_world()
        batches = shard_batches(0, export.total_frames, self.batch)
        host_export(export, world, rank, batches, self.batch, max(4, min(self.batch + 8, (4 << 30)//export.frame_bytes)),
                    lambda first, count, buffer: self.build(first, count), self.render)

    def export_device(self, export: "ExportingHelper", mode: str, turbo: bool) -> None:
        """The north star's layout: one contiguous frame range per rank, resident in HBM, sent to rank 0 — over RCCL ("device"), or copied
        into rank 0's buffer through peer windows ("device-sdma", which falls back to RCCL for the whole group when the windows fail)"""
        import torch
        import torch.distributed as dist
        context = self.scene.context
        rank, world = rank_world()
        total = export.total_frames
        device = torch.device("cuda", context.device)
        first, last = shard_frames(total, world, rank)
        frames_here = total if rank == 0 else (last - first)
        sink_bytes = export.frame_bytes
        window, size = None, max(1, frames_here)*sink_bytes
        if mode == "device-sdma" and rank == 0:
            # peer windows: rank 0's buffer is ONE raw allocation (IPC handles name whole allocations), mapped by every rank
            window = context.alloc(size)
            resident = torch.as_tensor(DeviceArray(window, size), device=device)
        else:
            resident = torch.zeros(size, dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)                  # the fill runs on torch's stream, the renders on the context's
        if mode == "device-sdma":
            try:
                transfer = SdmaTransfer(world, rank, context, sink_bytes, window, probe_at=first*sink_bytes,
                                        probe_bytes=min(4096, max(0, last - first)*sink_bytes))
            except PeerWindowsUnavailable as unavailable:
                # decided by every rank together (the outcomes were all-gathered): the windows do not work here, the chunks travel
                # as RCCL point-to-point calls instead — the same resident buffers, nothing rendered yet
                if rank == 0:
                    print(f"shaderflow_amd: peer windows unavailable ({unavailable}): SHADERFLOW_SHARD=device-sdma falls back to device mode", flush=True)
                transfer = RangeTransfer(world, rank, device)
        else:
            transfer = RangeTransfer(world, rank, device)
        sink = SinkBatches(export, self.batch, count=0)    # the resident buffers are the sink frames' home

        def render(first_frame, count, view):
            sink.render(view.data_ptr(), count, self.render)
            context.synchronize()                       # the context's stream is not torch's: complete before the send
        emit = lambda view, count: export.pipe_device_frames(view.data_ptr(), sink_bytes, count, turbo=turbo)

        # a rank that raises mid-export must not leave the others waiting for its chunks, nor rank 0's whole-export allocation
        # and the peers' mappings behind: the outcome is exchanged, then every rank tears down
        failure: Optional[BaseException] = None
        try:
            contiguous_device_export(world, rank, total, self.batch, sink_bytes, self.build, render, emit, resident, transfer)
            export.drain()                              # `resident` outlives the queued reads
        except BaseException as error:
            failure = error
            transfer.abort()
        finally:
            sink.close()
            try:
                if isinstance(transfer, SdmaTransfer):
                    transfer.close()                        # the peers' mappings of the window
                    dist.barrier(group=transfer.control)    # every peer has closed its mapping
            finally:
                if window is not None:                      # (also after the fall-back to RCCL: the frames still live in the raw allocation)
                    del resident
                    context.synchronize()
                    context.free(window)
        if failure is not None:
            raise failure
        if rank != 0:
            export.frame = total
