"""
ClockLoop: the frame loop of scenes in which nothing but the clock moves (no reference equivalent).

`ShaderScene.next` (scene.py:456-479) updates every module and lets every program walk every module's `pipeline()` — ≈ 150 µs of
python per frame whatever the scene does. Scenes made only of stock modules whose `DynamicNumber`s are at rest — Multipass, MotionBlur,
Life, any layered / temporal feedback scene without python logic between frames — change, from one frame to the next, exactly:
the four clock uniforms (iTime, iTau, iDeltatime, iFrame: scene.py:687-703), `iLayer` per draw, and WHICH device texture sits
behind every sampler of a temporal texture after its `roll()` (texture.py:295-298, 351-381). This loop does that and nothing else
per frame: one `sfx_uniform_set_clock`, one `sfx_sampler_bind_many` per rolled texture matrix, the draws, the resolve, the read-out.
Same launches in the same order with the same uniform values as the frame loop, so the same frames byte for byte
(tests/test_gpu_multipass.py); anything it is not sure about takes the frame loop. The loops that put something in front of the frames'
passes — an audio tape, a piano, a staged video — run the same native sequence through a `FrameSource` and `run_source` (sequence.py).
"""
from __future__ import annotations

import ctypes as C
from typing import TYPE_CHECKING, Optional

import numpy as np

from shaderflow_amd import _native as N
from shaderflow_amd.camera import CameraMode, ShaderCamera
from shaderflow_amd.dynamics import ShaderDynamics
from shaderflow_amd.module import ShaderModule
from shaderflow_amd.scheduler import freewheel_clock
from shaderflow_amd.shader import ShaderProgram
from shaderflow_amd.texture import ShaderTexture

if TYPE_CHECKING:
    from shaderflow_amd.exporting import ExportingHelper
    from shaderflow_amd.scene import ShaderScene


def box_handles(texture: ShaderTexture):
    """The device textures behind a matrix' samplers, in the order of `boxes`, as a C array"""
    return (N.Handle*(texture.temporal*texture.layers))(*[box.texture.handle if box.texture is not None else N.Handle() for (_, _, box) in texture.boxes])


def end_clock(policy: str, fps: float, speed: float, done: int) -> tuple[float, float, float]:
    """(time, dt, rdt) a loop leaves on the scene behind `done` >= 1 frames; the three loops differ on purpose, and tests pin them.
    "last": the last frame drawn (ClockLoop); "last_dt": the same with rdt = dt, as FrameTape.export leaves it (TapeSequence); "next": what
    scene.next leaves behind the last frame — it integrates time AFTER the frame (reference scene.py:475-479), so what a frame more
    would have seen (a Sequence with a piano or a video). sequence.ROWS says which sequence leaves which."""
    times, dts, rdts = freewheel_clock(fps, done + 1, speed)
    if policy == "next":
        return times[done], dts[done], rdts[done]
    last = done - 1
    return times[last], dts[last], {"last": rdts, "last_dt": dts}[policy][last]


class FrameSource:
    """What feeds sfx_sequence_run beside the clock: an audio tape, a piano, a staged video (tapesequence.py, pianosequence.py,
    videosequence.py), or several of them joined (JoinedSource; sequence.py's Sequence). `run_native` calls batches … consumed of its source, `run_source` the rest; as they stand here they do nothing,
    and that is the clock loop's own source."""
    end = "last"                                                       # the clock behind the run (end_clock)
    chunked = True                                                     # the loop's gate saw to it that every chunk can be ONE native call; False: native_sequence is asked

    def prepare(self, times, dts, total): pass                        # in front of `prime`: the device objects, what the run needs for every frame
    def batches(self, total): return [(0, total)]                     # the frame ranges (first, size) the run is cut into; a chunk stays inside one
    def begin_batch(self, first, size): pass
    def attach(self, sequence): pass                                  # the descriptor fields that hold for the whole run
    def take(self, sequence, first, count, batch_first): return count  # … and those of the call that draws `count` frames from `first`; it may shorten the call
    def consumed(self, first, count): pass                            # behind a native call that succeeded
    def settle(self, done): pass                                      # behind the run, however it ended: the host objects as the frame loop leaves them after `done` frames
    def finished(self, done, total): return True                      # whether a run_native that returned ran to its end (else a read-back error in `settle` is dropped)
    def release(self): pass


class JoinedSource(FrameSource):
    """Several frame sources in front of the same frames (sequence.py: a piano and its sound track), in the order given. Every call
    goes to every part in that order, `release` in reverse. At most one part may cut the run into batches (the tape), and a part whose
    `take` shortens a call must be the last: what the parts in front of it set for the call must not have depended on the longer count.
    `settle` reaches every part even when one raised; the first exception is raised again behind the last. `end` and `chunked` are the
    owner's to say: they belong to the loop, not to a part."""

    def __init__(self, parts, end: str = FrameSource.end, chunked: bool = FrameSource.chunked):
        self.parts = list(parts)
        self.end, self.chunked = end, chunked
        cutting = [part for part in self.parts if type(part).batches is not FrameSource.batches]
        if len(cutting) > 1:
            raise ValueError(f"{len(cutting)} frame sources cut the run into batches of their own: {', '.join(type(part).__name__ for part in cutting)}")
        self.cutting = cutting[0] if cutting else None

    def prepare(self, times, dts, total):
        for part in self.parts:
            part.prepare(times, dts, total)

    def batches(self, total):
        return self.cutting.batches(total) if self.cutting is not None else FrameSource.batches(self, total)

    def begin_batch(self, first, size):
        for part in self.parts:
            part.begin_batch(first, size)

    def attach(self, sequence):
        for part in self.parts:
            part.attach(sequence)

    def take(self, sequence, first, count, batch_first):
        for k, part in enumerate(self.parts):
            taken = part.take(sequence, first, count, batch_first)
            assert 0 < taken <= count and (taken == count or k == len(self.parts) - 1), \
                f"{type(part).__name__}.take shortened the call to {taken} of {count} frames in front of another source"
            count = taken
        return count

    def consumed(self, first, count):
        for part in self.parts:
            part.consumed(first, count)

    def settle(self, done):
        failure = None
        for part in self.parts:
            try:
                part.settle(done)
            except Exception as error:
                failure = failure or error
        if failure is not None:
            raise failure

    def finished(self, done, total):
        return all(part.finished(done, total) for part in self.parts)

    def release(self):
        for part in reversed(self.parts):
            part.release()


class ClockLoop:
    attribute = None                                                   # ShaderScene.main keeps no clock loop behind the run

    @staticmethod
    def applicable(scene: "ShaderScene", export: "Optional[ExportingHelper]" = None, turbo: bool = True, taped: frozenset = frozenset()) -> bool:
        """`taped`: ids of the modules a sequence computes for the caller (sequence.py) — left to its own judgement"""
        from shaderflow_amd.scene import ShaderScene
        if type(scene).update is not ShaderModule.update:
            return False
        # a scene with a frame step, a message handler or scheduled tasks of its own keeps the ordinary loop (this one runs none of them)
        if type(scene).next is not ShaderScene.next or type(scene).handle is not ShaderScene.handle:
            return False
        if any(task is not scene.vsync for task in scene.scheduler.tasks):
            return False
        if type(scene).pipeline is not ShaderScene.pipeline and not ClockLoop.pipeline_is_static(scene):
            return False
        for module in scene.modules:
            if module is scene or isinstance(module, ShaderScene) or id(module) in taped:
                continue
            if type(module) not in (ShaderCamera, ShaderDynamics, ShaderProgram, ShaderTexture):
                return False
            if isinstance(module, ShaderCamera) and module.mode == CameraMode.Spherical:
                return False                                          # align() runs every update() there and may move rotation.target again (camera.py:220-236)
            if isinstance(module, ShaderDynamics):
                # at rest, and staying there: the early-out of dynamics.py:222-225 — and no integral that keeps running
                value, target = np.asarray(module.value), np.asarray(module.target)
                if module.integrate or value.shape != target.shape or value.dtype.kind not in "fiu":
                    return False
                if value.size and float(np.abs(target - value).max()) >= module.precision:
                    return False
        return True

    CLOCK = ("iTime", "iTau", "iDeltatime", "iFrame")

    @staticmethod
    def pipeline_is_static(scene: "ShaderScene") -> bool:
        """A scene that overrides pipeline() to ADD uniforms (demo.py's Life: `iLifePeriod`): fine as long as what it adds does not move
        with the clock — asked the way the frame loop asks, by calling pipeline(), at two different times"""
        def snapshot():
            out = []
            for variable in scene.pipeline():
                if variable.name in ClockLoop.CLOCK:
                    continue
                value = variable.value
                if isinstance(value, np.ndarray):
                    value = (value.dtype.str, value.shape, value.tobytes())
                elif isinstance(value, (list, tuple)):
                    value = tuple(float(v) if isinstance(v, (int, float, np.number)) else repr(v) for v in value)
                elif not isinstance(value, (int, float, str, bool, type(None))):
                    value = id(value)                                  # a texture: the same object or not
                out.append((variable.type, variable.name, value))
            return out
        saved = (scene.time, scene.dt, scene.rdt)
        try:
            first = snapshot()
            scene.time, scene.dt, scene.rdt = saved[0] + 1.2345, 0.0173, 0.0173
            second = snapshot()
        except Exception:
            return False
        finally:
            scene.time, scene.dt, scene.rdt = saved
        return first == second

    def __init__(self, scene: "ShaderScene"):
        self.scene = scene
        self.programs = [m for m in reversed(scene.modules) if isinstance(m, ShaderProgram)]      # the order scene.next renders them in
        # texture matrices whose samplers move every frame, and their sampler names as a C array in the order of `boxes`, by id(texture):
        # the names never change
        self.rolling = [m for m in scene.modules if isinstance(m, ShaderTexture) and m.name and m.temporal > 1]
        self.sampler_names = {id(texture): (C.c_char_p*(texture.temporal*texture.layers))(*[texture._sampler_name(t, l).encode() for (t, l, _) in texture.boxes])
                              for texture in self.rolling}

    def bind_rolled(self, program: ShaderProgram) -> None:
        for texture in self.rolling:
            names = self.sampler_names[id(texture)]
            N.check(N.lib().sfx_sampler_bind_many(program.program, names, box_handles(texture), len(names)))

    # the same loop without python between the frames (csrc/capi.hip sfx_sequence_run) ---------------------------------------------------

    CHUNK = 240                                                        # most frames per native call: the encoder and `scene.quit` are looked at in between
    CHUNK_SECONDS = 0.25                                               # … and about how long a call may keep the host: the chunk is sized by the measured frame time

    def chunk_frames(self, measured: "float | None") -> int:
        """Frames of the next native call: CHUNK while nothing is known, then what fits CHUNK_SECONDS at the rate the last call ran at — a 4K
        frame that waits for its ring slot takes 0.5 ms, so 240 of them held scene.quit, the encoder check and Ctrl-C for 120 ms at best and
        for as long as the sink stalls at worst"""
        if not measured or measured <= 0.0:
            return min(self.CHUNK, 30)
        return max(1, min(self.CHUNK, int(self.CHUNK_SECONDS/measured)))

    def native_sequence(self, export: "ExportingHelper", turbo: bool) -> bool:
        """Whether the frames can be rendered, rolled, resolved, read out and piped by ONE native call per chunk: a turbo export without a
        progress relay (a relay wants a python call per frame), every program compiled. SHADERFLOW_CLOCK_SEQUENCE=0 keeps the python loop
        (A/B measurements, and the byte-equality test of the two)."""
        import os
        if os.environ.get("SHADERFLOW_CLOCK_SEQUENCE", "1") == "0" or not turbo or export.relay is not None or export.sized:
            return False
        return all(program.program is not None for program in self.programs)

    def run_native(self, export: "ExportingHelper", times, dts, rdts, total: int, source: "Optional[FrameSource]" = None, pipe_here: bool = False, turbo: bool = True) -> None:
        """Every chunk of frames is one sfx_sequence_run; what a `source` puts in front of the frames' passes it names in the descriptor
        itself (FrameSource). The frames go in the source's batches, in chunks that stay inside a batch. `pipe_here`: one frame per
        call, read out by export.pipe (a progress relay, no turbo)."""
        scene, lib, source = self.scene, N.lib(), source or FrameSource()
        runtime, fps = scene.runtime, scene.fps
        # texture matrices: every program's own (its draws go to row 0) — the same objects `rolling` lists when they are temporal
        textures = [program.texture for program in self.programs]
        index = {id(texture): m for m, texture in enumerate(textures)}
        passes = (N.SequencePass*len(self.programs))()
        for k, program in enumerate(self.programs):
            if program.texture.final:
                passes[k] = N.SequencePass(N.Handle(), N.PASS_RESOLVE, index[id(scene.shader.texture)], program.texture.fbo.handle, 0, scene.subsample)
            elif program is scene.shader and scene._can_fuse(program):
                passes[k] = N.SequencePass(program.program, N.PASS_FUSED, index[id(program.texture)], scene._final.texture.fbo.handle, int(scene.ssaa), scene.subsample)
            else:
                passes[k] = N.SequencePass(program.program, N.PASS_LAYERS, index[id(program.texture)], N.Handle(), 0, 0)
        keep = []                                                      # ctypes arrays the structures point into

        def matrix_tables():
            tables = (N.SequenceMatrix*len(textures))()
            for m, texture in enumerate(textures):
                handles = box_handles(texture)
                keep.append(handles)
                tables[m] = N.SequenceMatrix(texture.temporal, texture.layers, handles, self.sampler_names.get(id(texture)))
            return tables
        planar = (C.c_void_p*len(export._yuv_slots))(*export._yuv_slots) if export._yuv_slots else None      # (staging exists for a planar sink only)
        piping = export.fileno is not None and export.ring is not None and not pipe_here
        # what a run keeps: the passes, the sink and what the source attaches; every chunk sets the clock, the matrices and where it starts
        sequence = N.Sequence(passes=passes, npasses=len(self.programs), nmatrices=len(textures),
                              ring=export.ring if piping else N.Handle(), fd=export.fileno if piping else -1, planar_slots=planar,
                              yuv_matrix=1 if export.yuv_matrix == "bt709" else 0, width=scene.width, height=scene.height)
        source.attach(sequence)
        done = 0
        per_frame = None                                               # seconds per frame of the last native call
        import time as clock
        for first, size in source.batches(total):
            if scene.quit:
                break
            source.begin_batch(first, size)
            while done < first + size and not scene.quit:
                count = 1 if pipe_here else min(self.chunk_frames(per_frame), first + size - done)
                export._check_encoder()
                count = source.take(sequence, done, count, first)      # (may wait: not part of the frames' measured time)
                started = clock.perf_counter()
                ticks = (N.ClockTick*count)()
                for i in range(count):
                    time = times[done + i]
                    ticks[i] = N.ClockTick(time, (time/runtime) % 1.0, dts[done + i], round(time*fps))
                sequence.clock, sequence.nframes, sequence.matrices = ticks, count, matrix_tables()
                sequence.first_slot = export.frame % max(1, export.slots)
                N.check(lib.sfx_sequence_run(scene.context.handle, C.byref(sequence)))
                per_frame = (clock.perf_counter() - started)/count
                source.consumed(done, count)
                for texture in textures:
                    texture.roll(count)                               # the native call rolled its own copy of every matrix it drew into
                if pipe_here:
                    export.pipe(turbo=turbo)
                    export.update()
                else:
                    export.frame += count
                done += count
                keep.clear()

    def run_source(self, export: "ExportingHelper", source: "FrameSource", turbo: bool = True):
        """The export of a loop that feeds the native sequence (sequence.py). Whatever ends the
        run — the last frame, scene.quit, an encoder that died, a device error — the source settles the host objects at the last frame
        that was drawn, and the clock is the one its loop leaves there (`end_clock`)."""
        scene, total = self.scene, export.total_frames
        times, dts, rdts = freewheel_clock(scene.fps, total, scene.speed)
        try:
            source.prepare(times, dts, total)
            self.prime(times, dts, rdts)
            returned = False
            try:
                self.run_native(export, times, dts, rdts, total, source, not (source.chunked or self.native_sequence(export, turbo)), turbo)
                returned = True
            finally:
                self.forget_sent()
                done = min(total, export.frame)
                try:
                    source.settle(done)
                except N.NativeError:
                    if returned and source.finished(done, total):      # (behind a failed run the device may not answer: the first error is the one to report)
                        raise
                if done:
                    scene.time, scene.dt, scene.rdt = end_clock(source.end, scene.fps, scene.speed, done)
            return export.finish()
        finally:
            scene.context.synchronize()
            source.release()

    def prime(self, times, dts, rdts) -> None:
        """Frame 0's state through the ordinary pipeline walk: every uniform and sampler of every program is on the device"""
        scene = self.scene
        scene.time, scene.dt, scene.rdt = times[0], dts[0], rdts[0]
        for program in self.programs:
            if program.program is None:
                program.compile()
            if not program.texture.final:
                program.use_scene_pipeline()

    def forget_sent(self) -> None:
        """Behind a run: what the loop sent behind the programs' backs — their caches of sent values say something older"""
        for program in self.programs:
            program.forget_sent()

    def run(self, export: "ExportingHelper", turbo: bool):
        scene = self.scene
        total = export.total_frames
        times, dts, rdts = freewheel_clock(scene.fps, total, scene.speed)
        self.prime(times, dts, rdts)
        native = self.native_sequence(export, turbo)
        try:
            if native:
                self.run_native(export, times, dts, rdts, total)
            else:
                lib, runtime, fps = N.lib(), scene.runtime, scene.fps
                for k in range(total):
                    if scene.quit:                                    # ShaderMessage.Window.Close (scene.py:478-480), as the vsync loop honours it
                        break
                    time = times[k]
                    scene.time, scene.dt, scene.rdt = time, dts[k], rdts[k]
                    scene._fused_this_frame = False
                    for program in self.programs:
                        if not program.texture.final:
                            N.check(lib.sfx_uniform_set_clock(program.program, time, (time/runtime) % 1.0, dts[k], round(time*fps)))
                            self.bind_rolled(program)
                        program.render(pipeline=False)
                    export.pipe(turbo=turbo)
                    export.update()
        finally:
            self.forget_sent()
        if not native:
            scene.time, scene.dt, scene.rdt = times[-1], dts[-1], rdts[-1]      # the clock of the last frame
        elif export.frame:
            scene.time, scene.dt, scene.rdt = end_clock(FrameSource.end, scene.fps, scene.speed, min(total, export.frame))
        return export.finish()
