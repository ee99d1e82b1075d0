"""
VideoSequence: the staged video in front of the frames of video scenes without python logic (no reference equivalent).

`ShaderVideo.update()` (video.py) runs on the host for every source frame: the next array from a python iterator, a flipped contiguous
host copy of it (6.2 MB at 1080p, 24.9 MB at 4K), a synchronous upload, and only then the draw. No fast loop knew the module, so a scene
with a video always took `ShaderScene.next`, frame by frame, nothing overlapping.

Here source frames are staged ahead of the draws: a reader thread fills pinned slots in source order (`file.readinto` / a memory-mapped
copy straight into the slot, both without the GIL) and submits each one's asynchronous host → device copy on the stage's own copy
stream (`sfx_video_submit`). ClockLoop's native sequence draws the frames in chunks (`sfx_sequence_run` with the video named, by this class
as its `FrameSource`): in front of
the first pass of every scene frame a source frame lands on, the render stream waits for that slot's copy, the video's texture matrix
rolls and one launch of `k_video_frame` (csrc/video_kernels.hpp) writes the frame into the front box — rows flipped, and converted from
4:2:0 when the source is planar. The frames are the frame loop's byte for byte.

Which scene frame lands which source frame is host arithmetic (`landing_frames`): `update()`'s own test, `scene.time > frames_read/fps`,
walked over the export's clock. Slots are bounded (`slot_count`): at most SLOT_BYTES of pinned memory, and as much device staging; a
chunk consumes at most half of them, so the next chunk's reads and copies overlap this chunk's draws.

Behind a run — finished, quit or failed — the host objects are where the frame loop leaves them after the last frame drawn: `_read`,
`_exhausted`, the texture's host copies (read back from the device) and the clock; frames the reader took from the source ahead of the
draws go back in front of it for a later `update()`.

Which scenes run this way, alone or beside audio modules or a piano, is `Sequence`'s to say (sequence.py). Out of scope, so they keep
the frame loop: several videos, `layers != 1`, a subclass of ShaderVideo, sharded runs and a scene `update()` of its own. Planar
sources of every layout (`video.format == "planar"`: planarsource.py) land through `k_video_planar` where `k_video_frame` would run.

Motion-JPEG sources (`video.format == "mjpeg"`: mjpegsource.py) stay compressed in the slots: the reader stages each JPEG stream
(`mjpegsource.stage`: tables, interval starts, scan), only those bytes are copied, and a landing launches the decode kernels
(csrc/jpeg_decode_kernels.hpp) instead of `k_video_frame`. `slot_count` works from the slots' capacity; frames taken ahead go back in
front of the source as the `bytes` they came as; a frame the device could not decode fails the export with RuntimeError naming the
source frame (`undecoded`; found behind the last chunk, it is raised once the export is finished), and the context stays usable.
PNG sources (`video.format == "png"`: pngsource.py) go the same way, with `pngsource.stage` and the PNG kernels (csrc/png_decode_kernels.hpp).
"""
from __future__ import annotations

import ctypes as C
import itertools
import threading
from typing import TYPE_CHECKING, Optional

import numpy as np

from shaderflow_amd.clockloop import ClockLoop, FrameSource
from shaderflow_amd.module import logger
from shaderflow_amd.video import ShaderVideo, VideoStage

if TYPE_CHECKING:
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


def video_fits(video: ShaderVideo) -> bool:
    """Whether this video's texture is what k_video_frame writes (VideoSequence, alone or beside other sources): one
    layer of RGB8 of the clip's own size that follows no resolution, every box on the device"""
    texture = video.texture
    if texture is None or texture.layers != 1 or texture.components != 3 or texture.dtype != np.uint8:
        return False
    return not texture.track and texture.size == (video.width, video.height) and all(box.texture is not None for (_, _, box) in texture.boxes)


class VideoSequence(FrameSource):
    def __init__(self, scene: "ShaderScene", clock: ClockLoop):
        self.scene = scene
        self.clock = clock                                             # the run's (sequence.py): the sampler names of the video's matrix
        self.video = next(m for m in scene.modules if type(m) is ShaderVideo)
        self.stage: Optional[VideoStage] = None
        self.landed = 0                                                # source frames those frames landed
        self.lock = threading.Condition()
        self.thread: Optional[threading.Thread] = None

    # the frame source: a staged source frame goes in front of the frames that land one ------------------------------------------------

    def attach(self, sequence) -> None:
        # the sampler names of the matrix' rows, depth 0 first, when it is temporal (else None: the host's bindings stay)
        sequence.video, sequence.video_names = self.stage.handle, self.clock.sampler_names.get(id(self.video.texture))

    def take(self, sequence, first: int, count: int, batch_first: int) -> int:
        """The slot table of the native call that starts at scene frame `first`: up to `count` frames, shortened so that its landings
        are staged already and fill at most half the slots. Waits for the reader only when the call's first frame needs a frame that is
        not there yet; a reader that failed raises its exception here, once the frames staged before it failed are drawn."""
        slots = np.full(count, -1, np.int32)
        landings = 0
        for i in range(count):
            source = int(self.want[first + i])
            if source < 0:
                continue
            slot = -1                                                 # (half the slots are taken: as if not staged yet)
            if landings < self.per_chunk:
                with self.lock:
                    slot = self.await_frame(source, first + i, wait=(i == 0))
            if slot is None:                                          # the source ended in front of this frame: it shows what was there
                continue
            if slot < 0:                                              # not staged yet: the call ends in front of this frame
                count = i
                break
            slots[i] = slot
            landings += 1
        self.landing = slots[:count]
        sequence.video_slots = self.landing.ctypes.data_as(C.POINTER(C.c_int32))
        return count

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

    def consumed(self, first: int, count: int) -> None:
        """The native call has queued these landings: their slots go back to the reader (it waits for each kernel before it refills)"""
        slots = self.landing
        used = [int(slot) for slot in slots if slot >= 0]
        with self.lock:
            for i in range(count):
                if slots[i] >= 0:
                    self.staged.pop(int(self.want[first + i]), None)
                    self.held.pop(int(self.want[first + i]), None)
            self.free.extend(used)
            self.landed += len(used)
            self.lock.notify_all()
        self.video.texture.roll(len(used))                            # the native call rolled its own copy of the matrix once per landing
        error = self.undecoded(wait=False)
        if error is not None:
            self.error = error
            raise error

    def undecoded(self, wait: bool) -> Optional[RuntimeError]:
        """A compressed frame the device could not decode fails the export: the error that says so, or None (the kernels noted the
        first such frame; asking costs no wait unless `wait` says so: a damaged frame is then found a chunk later, or behind the run)"""
        bad = self.stage.bad_frame(wait) if self.stage is not None else None      # (an uncompressed frame is never bad, and nothing waits for one)
        if bad is None:
            return None
        return RuntimeError(f"{self.video.name}: source frame {self.first_read + bad[0]} could not be decoded: {self.stage.describe_status(bad[1])}")

    def raise_undecoded(self) -> None:
        """Behind `run_source`: a damaged frame that only `settle`'s waiting check found. The run drew every frame, so the clock is
        set and the export finished (a sink's file is whole) before the error leaves."""
        if self.late is not None:
            raise self.late

    # the reader ------------------------------------------------------------------------------------------------------------------------

    def read_frames(self, source, first: int, needed: int) -> None:
        """The reader thread: source frames first, first + 1, … into free slots, each submitted as soon as it is whole"""
        stage, video = self.stage, self.video
        readinto = getattr(source, "readinto", None) if stage.planar else None
        try:
            for index in range(first, first + needed):
                with self.lock:
                    while not self.free and not self.stop:
                        self.lock.wait(0.05)
                    if self.stop:
                        return
                    slot = self.free.pop(0)
                view = stage.view(slot)                               # (waits for the kernel that consumed the slot's last frame)
                size, held = None, view                               # `held`: what `put_back` gets should nobody draw the frame
                if readinto is not None:
                    whole = readinto(view)
                else:
                    try:
                        frame = next(source)
                    except StopIteration:
                        whole = False
                    else:
                        size = stage.fill(view, frame, f"{video.name}: source frame {index}")
                        held = view if size is None else frame        # (a frame with a size of its own came as a stream: that goes back)
                        whole = True
                with self.lock:
                    if not whole:
                        self.free.append(slot)
                        self.total = index
                        self.lock.notify_all()
                        return
                    if self.stop:                                     # (the frame is whole but nobody will draw it: it goes back to the source)
                        self.kept[index] = stage.put_back(held)
                        return
                stage.submit(slot, size)
                with self.lock:
                    self.staged[index] = slot
                    self.held[index] = held
                    self.lock.notify_all()
        except BaseException as error:                                # whatever the source raised fails the export, in the thread that drives it
            with self.lock:
                self.error = error
                self.lock.notify_all()

    # the export ------------------------------------------------------------------------------------------------------------------------

    def prepare(self, times, dts, total: int) -> None:
        """The stage and the reader thread"""
        video = self.video
        self.first_read, self.was_exhausted, self.source = video._read, video._exhausted, video._reader
        # every landing of the export, were the source endless; where it ends is learnt from the reader
        self.want = landing_frames(times, video.fps, self.first_read) if not self.was_exhausted else np.full(total, -1, np.int64)
        self.stage = VideoStage(video, slot_count)
        slots = self.stage.slots
        self.per_chunk = slots//2
        self.free, self.staged, self.held, self.kept = list(range(slots)), {}, {}, {}   # held: source frame → its stream, or its slot's view
        self.total, self.error, self.late, self.stop, self.exhausted_at = None, None, None, False, None
        self.landed = 0
        self.thread = threading.Thread(target=self.read_frames, args=(self.source, self.first_read, int((self.want >= 0).sum())),
                                       name="shaderflow-video-reader", daemon=True)
        self.thread.start()

    def settle(self, done: int) -> None:
        video = self.video
        with self.lock:
            self.stop = True
            self.lock.notify_all()
        self.thread.join()
        video._read = self.first_read + self.landed
        video._exhausted = self.was_exhausted or (self.exhausted_at is not None and self.exhausted_at < done)
        if video._exhausted and not self.was_exhausted:
            logger.warning(f"{video.name}: source ended after {video._read} frames, holding the last one")
        # frames taken from the source but not drawn go back in front of it, in order, for a later update()
        ahead = {index: self.stage.put_back(self.held[index]) for index in self.staged}
        ahead.update(self.kept)
        if ahead:
            video._reader = itertools.chain([ahead[index] for index in sorted(ahead)], self.source)
        # the host copies of the boxes the run wrote into, as `texture.write` keeps them: read back from the device
        for depth in range(min(self.landed, video.texture.temporal) if done else 0):
            video.texture.refresh_host_copy(depth)
        if self.error is None:
            self.late = self.undecoded(wait=True)

    def finished(self, done: int, total: int) -> bool:
        return self.error is None and not self.scene.quit and done == total

    def release(self) -> None:
        if self.stage is not None:
            self.stage.release()
            self.stage = None
        self.held = {}
