"""
VideoSequence: the frame loop of video scenes without python logic (no reference equivalent).

`ShaderVideo.update()` (video.py) runs on the host for every source frame: the next array from a python iterator, a flipped contiguous
host copy of it (6.2 MB at 1080p, 24.9 MB at 4K), a synchronous upload, and only then the draw. No fast loop knew the module, so a scene
with a video always took `ShaderScene.next`, frame by frame, nothing overlapping.

Here source frames are staged ahead of the draws: a reader thread fills pinned slots in source order (`file.readinto` / a memory-mapped
copy straight into the slot, both without the GIL) and submits each one's asynchronous host → device copy on the stage's own copy
stream (`sfx_video_submit`). ClockLoop's native sequence draws the frames in chunks (`sfx_sequence_run` with the video named): in front of
the first pass of every scene frame a source frame lands on, the render stream waits for that slot's copy, the video's texture matrix
rolls and one launch of `k_video_frame` (csrc/video_kernels.hpp) writes the frame into the front box — rows flipped, and converted from
4:2:0 when the source is planar. The frames are the frame loop's byte for byte.

Which scene frame lands which source frame is host arithmetic (`landing_frames`): `update()`'s own test, `scene.time > frames_read/fps`,
walked over the export's clock. Slots are bounded (`slot_count`): at most SLOT_BYTES of pinned memory, and as much device staging; a
chunk consumes at most half of them, so the next chunk's reads and copies overlap this chunk's draws.

Behind a run — finished, quit or failed — the host objects are where the frame loop leaves them after the last frame drawn: `_read`,
`_exhausted`, the texture's host copies (read back from the device) and the clock; frames the reader took from the source ahead of the
draws go back in front of it for a later `update()`.

A scene takes this loop when `main(batch=None)` finds it applicable (after ClockLoop, before PianoSequence) and
`SHADERFLOW_VIDEO_SEQUENCE` is not "0". Out of scope, so they keep the frame loop: a video beside audio or piano modules
(`sfx_sequence_run` refuses the combination), several videos, `layers != 1`, a subclass of ShaderVideo, sharded runs, a scene `update()`
of its own, and — for the planar sources — bt709 or full-range input, chroma interpolation and 10-bit sources (the reader refuses what
it can see of them).
"""
from __future__ import annotations

import ctypes as C
import itertools
import os
import threading
from typing import TYPE_CHECKING, Optional

import numpy as np

from shaderflow_amd import _native as N
from shaderflow_amd.clockloop import ClockLoop
from shaderflow_amd.module import logger
from shaderflow_amd.parallel import is_sharded
from shaderflow_amd.scheduler import freewheel_clock
from shaderflow_amd.video import ShaderVideo, VideoStage

if TYPE_CHECKING:
    from shaderflow_amd.exporting import ExportingHelper
    from shaderflow_amd.scene import ShaderScene

SLOT_BYTES = 256 << 20                                                 # pinned staging of one run, at most (and as much on the device)
SLOTS_MIN, SLOTS_MAX = 4, 32


def slot_count(frame_bytes: int) -> int:
    """Pinned slots of a run: what fits SLOT_BYTES, an even number between SLOTS_MIN and SLOTS_MAX (4K rgb24: 10 slots = 249 MB)"""
    return max(SLOTS_MIN, min(SLOTS_MAX, SLOT_BYTES//max(1, frame_bytes)))//2*2


def landing_frames(times, fps: float, first_read: int = 0, available: Optional[int] = None) -> np.ndarray:
    """Which source frame every scene frame lands: out[k] = r when `update()` at scene.time = times[k] reads source frame r (video.py:100:
    `scene.time > read/fps` with `read` frames read so far, starting at `first_read`), -1 when the frame shows what was there. At most
    one frame lands per scene frame. `available`: how many frames the source holds in all (None: unknown, never ending) — nothing lands
    once a read has failed."""
    out = np.full(len(times), -1, np.int64)
    read = int(first_read)
    for k, time in enumerate(times):
        if not (time > (read/fps)):
            continue
        if available is not None and read >= available:
            break                                                     # StopIteration: `_exhausted`, the last frame is held
        out[k] = read
        read += 1
    return out


class VideoSequence:
    @staticmethod
    def applicable(scene: "ShaderScene", export: "ExportingHelper | None" = None, turbo: bool = True) -> bool:
        if os.environ.get("SHADERFLOW_VIDEO_SEQUENCE", "1") == "0":
            return False
        if not scene.freewheel or is_sharded() or not turbo or (export is not None and export.relay is not None):
            return False
        videos = [m for m in scene.modules if isinstance(m, ShaderVideo)]
        if len(videos) != 1 or type(videos[0]) is not ShaderVideo:     # (a subclass may update() differently from what the sequence schedules)
            return False
        video = videos[0]
        texture = video.texture
        if texture is None or texture.layers != 1 or texture.components != 3 or texture.dtype != np.uint8:
            return False
        if texture.track or texture.size != (video.width, video.height) or any(box.texture is None for (_, _, box) in texture.boxes):
            return False
        # everything else must be what ClockLoop takes: no python logic, no audio modules, no piano, no other module type
        if not ClockLoop.applicable(scene, taped=frozenset(id(m) for m in (video, texture))):
            return False
        from shaderflow_amd.shader import ShaderProgram
        return all(m.program is not None for m in scene.modules if isinstance(m, ShaderProgram))

    def __init__(self, scene: "ShaderScene"):
        self.scene = scene
        self.clock = ClockLoop(scene)                                  # the pass and matrix tables, the chunk size
        self.video = next(m for m in scene.modules if type(m) is ShaderVideo)
        self.stage: Optional[VideoStage] = None
        self.frames = 0                                                # frames drawn by the native sequence (tests, measurements)
        self.landed = 0                                                # source frames those frames landed
        self.lock = threading.Condition()
        self.thread: Optional[threading.Thread] = None

    # what run_native asks of its `video` -----------------------------------------------------------------------------------------------

    @property
    def handle(self):
        return self.stage.handle

    @property
    def names(self):
        """The sampler names of the matrix' rows, depth 0 first, when it is temporal (else None: the host's bindings stay)"""
        texture = self.video.texture
        if not texture.name or texture.temporal < 2:
            return None
        return (C.c_char_p*texture.temporal)(*[texture._sampler_name(t, 0).encode() for t in range(texture.temporal)])

    def take(self, first: int, count: int):
        """(frames, slot table) of the native call that starts at scene frame `first`: up to `count` frames, shortened so that its landings
        are staged already and fill at most half the slots. Waits for the reader only when the call's first frame needs a frame that is
        not there yet; a reader that failed raises its exception here, once the frames staged before it failed are drawn."""
        slots = np.full(count, -1, np.int32)
        landings = 0
        for i in range(count):
            source = int(self.want[first + i])
            if source < 0:
                continue
            if landings >= self.per_chunk:
                return i, slots[:i]
            with self.lock:
                slot = self.await_frame(source, first + i, wait=(i == 0))
            if slot is None:                                          # the source ended in front of this frame: it shows what was there
                continue
            if slot < 0:                                              # not staged yet: the call ends in front of this frame
                return i, slots[:i]
            slots[i] = slot
            landings += 1
        return count, slots

    def await_frame(self, source: int, frame: int, wait: bool):
        """The slot source frame `source` is staged in; None when the source ended before it; -1 when it is not there yet and the caller
        does not `wait` (called with the lock held)"""
        while True:
            if source in self.staged:
                return self.staged[source]
            if self.total is not None and source >= self.total:
                self.end_of_source(frame)
                return None
            if self.error is not None:
                if wait:
                    raise self.error
                return -1
            if not wait:
                return -1
            if not self.thread.is_alive():
                raise RuntimeError("video sequence: the reader ended without a frame, an end of the source or an error")
            self.lock.wait(0.05)

    def end_of_source(self, frame: int) -> None:
        """The source ended in front of the frame scene frame `frame` wanted: nothing lands from there on (called with the lock held)"""
        self.want[self.want >= self.total] = -1
        if self.exhausted_at is None:
            self.exhausted_at = frame

    def consumed(self, first: int, count: int, slots: np.ndarray) -> None:
        """The native call has queued these landings: their slots go back to the reader (it waits for each kernel before it refills)"""
        used = [int(slot) for slot in slots if slot >= 0]
        with self.lock:
            for i in range(count):
                if slots[i] >= 0:
                    self.staged.pop(int(self.want[first + i]), None)
            self.free.extend(used)
            self.landed += len(used)
            self.lock.notify_all()
        self.video.texture.roll(len(used))                            # the native call rolled its own copy of the matrix once per landing

    # the reader ------------------------------------------------------------------------------------------------------------------------

    def read_frames(self, source, first: int, needed: int) -> None:
        """The reader thread: source frames first, first + 1, … into free slots, each submitted as soon as it is whole"""
        stage, video = self.stage, self.video
        nbytes = video.width*video.height*3//(2 if video.format == "i420" else 1)
        readinto = getattr(source, "readinto", None) if video.format == "i420" else None
        try:
            for index in range(first, first + needed):
                with self.lock:
                    while not self.free and not self.stop:
                        self.lock.wait(0.05)
                    if self.stop:
                        return
                    slot = self.free.pop(0)
                view = stage.view(slot)                               # (waits for the kernel that consumed the slot's last frame)
                if readinto is not None:
                    whole = readinto(view)
                else:
                    try:
                        frame = next(source)
                    except StopIteration:
                        whole = False
                    else:
                        frame = np.asarray(frame, np.uint8)
                        if frame.size != nbytes:
                            raise ValueError(f"{video.name}: a frame of {video.width} x {video.height} has {nbytes} bytes, the source gave {frame.size}")
                        np.copyto(view.reshape(frame.shape), frame)   # (a memory-mapped clip is read here, without the GIL)
                        whole = True
                with self.lock:
                    if not whole:
                        self.free.append(slot)
                        self.total = index
                        self.lock.notify_all()
                        return
                    if self.stop:                                     # (the frame is whole but nobody will draw it: it goes back to the source)
                        self.kept[index] = view.copy()
                        return
                stage.submit(slot)
                with self.lock:
                    self.staged[index] = slot
                    self.views[slot] = view
                    self.lock.notify_all()
        except BaseException as error:                                # whatever the source raised fails the export, in the thread that drives it
            with self.lock:
                self.error = error
                self.lock.notify_all()

    # the export ------------------------------------------------------------------------------------------------------------------------

    def read_state(self, landed: int) -> None:
        """The host copies of the boxes the run wrote into, as `texture.write` keeps them: read back from the device"""
        texture = self.video.texture
        for depth in range(min(landed, texture.temporal)):
            box = texture.get_box(depth)
            box.data, box.empty = box.texture.read().tobytes(), False

    def run(self, export: "ExportingHelper", turbo: bool):
        scene, clock, video = self.scene, self.clock, self.video
        total = export.total_frames
        times, dts, rdts = freewheel_clock(scene.fps, total, scene.speed)
        first_read, was_exhausted = video._read, video._exhausted
        # every landing of the export, were the source endless; where it ends is learnt from the reader
        self.want = landing_frames(times, video.fps, first_read) if not was_exhausted else np.full(total, -1, np.int64)
        needed = int((self.want >= 0).sum())
        frame_bytes = video.width*video.height*3//(2 if video.format == "i420" else 1)
        slots = slot_count(frame_bytes)
        self.per_chunk = slots//2
        self.free, self.staged, self.views, self.kept = list(range(slots)), {}, {}, {}
        self.total, self.error, self.stop, self.exhausted_at = None, None, False, None
        self.landed = 0
        source = video._reader
        try:
            clock.prime(times, dts, rdts)
            self.stage = VideoStage(video, slots)
            self.thread = threading.Thread(target=self.read_frames, args=(source, first_read, needed), name="shaderflow-video-reader", daemon=True)
            self.thread.start()
            try:
                clock.run_native(export, times, dts, rdts, total, video=self)
            finally:
                clock.forget_sent()
                with self.lock:
                    self.stop = True
                    self.lock.notify_all()
                self.thread.join()
                # Whatever ended the run — the last frame, scene.quit, an encoder that died, a reader that raised — the host objects are
                # left at the last frame that was drawn
                self.frames = done = min(total, export.frame)
                video._read = first_read + self.landed
                video._exhausted = was_exhausted or (self.exhausted_at is not None and self.exhausted_at < done)
                if video._exhausted and not was_exhausted:
                    logger.warning(f"{video.name}: source ended after {video._read} frames, holding the last one")
                # frames taken from the source but not drawn go back in front of it, in order, for a later update()
                ahead = {index: self.views[slot].copy() for index, slot in self.staged.items()}
                ahead.update(self.kept)
                if ahead:
                    shape = (-1,) if video.format == "i420" else (video.height, video.width, 3)
                    video._reader = itertools.chain([ahead[index].reshape(shape) for index in sorted(ahead)], source)
                if done:
                    try:
                        self.read_state(self.landed)
                    except N.NativeError:
                        if self.error is None and not scene.quit and done == total:
                            raise
                    # the clock as scene.next leaves it behind the last frame (it integrates time AFTER the frame): what a frame more would have seen
                    after = freewheel_clock(scene.fps, done + 1, scene.speed)
                    scene.time, scene.dt, scene.rdt = after[0][done], after[1][done], after[2][done]
            return export.finish()
        finally:
            scene.context.synchronize()
            if self.stage is not None:
                self.stage.release()
                self.stage = None
            self.views = {}
