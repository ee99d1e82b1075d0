"""
ExportingHelper: frame counter, read-out ring and the encoder hand-off of an export.

Host mirror of the reference's shaderflow/exporting.py:30-203. The reference reads the final FBO into one of N
GL buffers (`fbo.read_into`) and lets turbopipe write it to ffmpeg's stdin from a worker thread; here the final
RGB8 texture is copied to one of N PINNED host buffers on a copy stream (`sfx_ring_read_async`) and a native
writer thread streams it to a file descriptor (`sfx_ring_pipe`), with the same reuse fence (`turbopipe.sync` →
`sfx_ring_pipe_sync`). Frames leave exactly as the reference hands them to ffmpeg: rgb24, rows BOTTOM-UP
(ffmpeg then applies `vflip`, exporting.py:94-103).

Sinks: a path ending in .rgb/.raw (or any path when no `ffmpeg` binary exists) receives the raw frames;
"pipe"/"-"/bytes returns them; with an `ffmpeg` binary on PATH other paths are encoded by the command line
`scene.ffmpeg` (shaderflow_amd/ffmpeg.py) builds exactly as the reference does: rawvideo rgb24 stdin, scale, vflip,
the configured codecs, `module.ffhook` additions such as the audio track (exporting.py:91-120).

Encoder hand-off on the device: when frames go to an ffmpeg process the resolve kernels write the
rows top-down (`sfx_ctx_output_top_down`) and the `vflip` filter is left out of the command, which takes a full
pass over every frame off the encoder's CPU threads. Raw sinks keep the reference's byte stream (rows bottom-up)
unless `top_down=True` is asked for.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import tempfile
import time
from pathlib import Path
from typing import TYPE_CHECKING, Any, Callable, Optional

import numpy as np
from attrs import Factory, define

from shaderflow_amd import _native as N
from shaderflow_amd import mjpeg
from shaderflow_amd.module import logger

if TYPE_CHECKING:
    from shaderflow_amd.scene import ShaderScene


@define(slots=False, eq=False)
class ExportingHelper:
    scene: "ShaderScene"

    frame: int = 0
    start: float = Factory(time.monotonic)
    relay: Optional[Callable[[int, int], None]] = None
    took: Optional[float] = None

    # sink
    kind: Optional[str] = None            # "path-raw", "path-ffmpeg", "path-mjpeg" (a file of sized frames: mjpeg or png), "pipe"
    path: Optional[Path] = None
    process: Optional[subprocess.Popen] = None
    file: Any = None
    fileno: Optional[int] = None
    top_down: Optional[bool] = None       # None: top-down exactly when an ffmpeg process is the sink
    pixel_format: str = "rgb24"
    """What the sink receives: "rgb24" — the reference's byte stream (exporting.py:97) — or "yuv420p": planar 4:2:0 made on the device
    (sfx_rgb_to_yuv420: BT.601 limited range, or `yuv_matrix = "bt709"`), half the bytes over PCIe and the pipe; ffmpeg takes it as
    `-pix_fmt yuv420p` rawvideo and the codec's own conversion falls away. Opt-in: `scene.main(pixel_format="yuv420p")`."""
    yuv_matrix: str = "bt601"
    _yuv_slots: list = Factory(list)      # device staging of the frame loop's converted frames, one per ring slot
    jpeg_quality: int = 90
    """`pixel_format="mjpeg"`: baseline JPEG frames encoded on the device (csrc/jpeg_kernels.hpp; mjpeg.py has the containers). The sink
    frames are of fixed capacity on the device and say how long they are; a sized ring reads out exactly their payload. No ffmpeg process."""
    container: Optional[str] = None       # of an mjpeg or png export to a path: "avi" or "raw" (mjpeg.container_of)
    _encoder: Any = None                  # N.JpegEncoder or N.PngEncoder
    _avi: Optional[mjpeg.AviWriter] = None
    _sizes: list = Factory(list)          # payload sizes of the mjpeg or png frames written, in order (the AVI index)
    sound_track: Any = False
    """An mjpeg or png export to `.avi` carries the scene's sound (mjpeg.py states the stream): True — the scene's one ShaderAudio that holds a
    loaded clip, from `file=` or `samples=` — or that module, or its name. The ring's writer thread puts each frame's share of the PCM
    behind the frame (sfx_ring_side_track): it alone orders the bytes on the sink's descriptor, in all three loops."""
    _track: Optional[mjpeg.SoundTrack] = None
    _track_ends: Optional[np.ndarray] = None   # the ring borrows it (and the track's pcm) until it is destroyed
    opendml: Any = None
    """An mjpeg or png export to `.avi` is written as OpenDML (AVI 2.0: `RIFF 'AVIX'` segments behind the first RIFF chunk, 64-bit `indx` /
    `ix##` indexes; mjpeg.py states the file), which holds exports past AVI 1.0's 4 GiB: True — segments of 1 GiB — or the segment size
    in bytes (4 096 … 2^31). The ring's writer thread leaves the gap in front of a segment's first frame (sfx_ring_segments), next to
    the side track's rule and for the same reason. None, False: the AVI 1.0 file, byte for byte as before."""
    _budget: Optional[int] = None              # the checked segment size of an OpenDML export
    _cuts: list = Factory(list)                # the frames in front of which the ring's writer left a gap (sfx_ring_segment_cuts)

    # ring
    ring: Optional[N.Handle] = None
    slots: int = 0

    @property
    def total_frames(self) -> int:
        return max(1, round(self.scene.runtime*self.scene.fps))

    @property
    def planar(self) -> bool:
        return self.pixel_format == "yuv420p"

    @property
    def mjpeg(self) -> bool:
        return self.pixel_format == "mjpeg"

    @property
    def png(self) -> bool:
        """`pixel_format="png"`: lossless — every frame a complete PNG file encoded on the device (csrc/png_kernels.hpp) — as the `00dc`
        chunks of an `.avi` file (fourcc `MPNG`) or back to back on a "pipe". A sink frame's capacity is the encoder's own bound
        (sfx_png_capacity): no frame can fail to fit. No ffmpeg process."""
        return self.pixel_format == "png"

    @property
    def sized(self) -> bool:
        """A sized-frame format: the sink frames say how long they are, a sized ring reads out their payload (mjpeg, png)"""
        return self.mjpeg or self.png

    @property
    def staged(self) -> bool:
        """Sink frames are made from the RGB8 frames by a kernel: into a batch buffer, or a staging frame of the ring slot"""
        return self.planar or self.sized

    @property
    def frame_bytes(self) -> int:
        """Bytes of one frame as the sink receives it (mjpeg, png: the fixed capacity of a sink frame on the device, its 64-byte header included)"""
        pixels = self.scene.width*self.scene.height
        if self.png:
            return N.PngEncoder.SINK_HEADER + N.PngEncoder.capacity(self.scene.width, self.scene.height)
        if self.mjpeg:
            return N.JpegEncoder.SINK_HEADER + ((self.scene.width + 15)//16)*((self.scene.height + 15)//16)*768
        return pixels*3//2 if self.planar else pixels*3

    @property
    def encoder(self):
        if self._encoder is None and self.png:
            self._encoder = N.PngEncoder(self.scene.context, self.scene.width, self.scene.height)
        if self._encoder is None:
            self._encoder = N.JpegEncoder(self.scene.context, self.scene.width, self.scene.height, self.jpeg_quality)
        return self._encoder

    def check(self, code: int) -> None:
        """N.check of a ring call; a frame the encoder could not fit into its sink frame is said in the export's words"""
        try:
            N.check(code)
        except N.NativeError as error:
            found = re.search(r"frame (\d+) does not fit", str(error))
            if self.mjpeg and error.code == N.E_TOO_LARGE and found:
                raise RuntimeError(f"frame {found.group(1)} does not fit at quality {self.jpeg_quality}") from None
            raise

    def to_yuv(self, rgb: int, yuv: int, frames: int = 1) -> None:
        self.scene.context.rgb_to_yuv420(rgb, yuv, self.scene.width, self.scene.height, frames, 1 if self.yuv_matrix == "bt709" else 0)

    def to_sink(self, rgb: int, target: int, frames: int = 1) -> None:
        """`frames` RGB8 frames on the device → sink frames at `target`, on the context's stream"""
        if self.planar:
            self.to_yuv(rgb, target, frames)
        elif self.sized:
            self.encoder.encode(rgb, target, frames, bottom_up=not self.top_down)
        else:
            self.scene.context.copy(target, rgb, frames*self.frame_bytes)

    @property
    def finished(self) -> bool:
        return (self.frame >= self.total_frames)

    def open_bar(self) -> None:
        self.start = time.monotonic()

    def update(self) -> None:
        if self.relay:
            self.relay(self.frame, self.total_frames)
        self.frame += 1

    # configuration --------------------------------------------------------------------------------------------

    @property
    def ffmpeg(self):
        return self.scene.ffmpeg

    def ffmpeg_clean(self) -> None:
        self.ffmpeg.clear(video_codec=False, audio_codec=False)

    def ffmpeg_sizes(self, width: int, height: int) -> None:
        self.ffmpeg.time = self.scene.runtime
        if self.pixel_format not in ("rgb24", "yuv420p", "mjpeg", "png"):
            raise ValueError(f"pixel_format {self.pixel_format!r}: 'rgb24' (the reference's stream), 'yuv420p' (converted on the device), 'mjpeg' (encoded on the device) "
                             f"or 'png' (lossless, encoded on the device)")
        if self.sized:
            if self.mjpeg:
                mjpeg.check_quality(self.jpeg_quality)
            return                                            # no encoder process: nothing to configure
        if self.planar and (self.scene.width % 2 or self.scene.height % 2):
            raise ValueError(f"yuv420p needs even extents, the scene is {self.scene.width}x{self.scene.height}")
        self.ffmpeg.pipe_input(pixel_format=self.pixel_format, width=self.scene.width, height=self.scene.height, framerate=self.scene.fps)
        self.ffmpeg.scale(width=width, height=height)
        self.ffmpeg.vflip()

    @property
    def wants_track(self) -> bool:
        return self.sound_track is not False and self.sound_track is not None

    def find_track(self) -> mjpeg.SoundTrack:
        """The clip `sound_track` names, as the file will hold it; ValueError when the export cannot hold one or the scene has none"""
        from shaderflow_amd.audio import ShaderAudio
        rule = "sound_track goes into an '.avi' file of a Motion-JPEG or PNG export (output='clip.avi', pixel_format='mjpeg' or 'png')"
        if not self.sized:
            raise ValueError(f"{rule}, not pixel_format {self.pixel_format!r}: the ffmpeg branch already attaches the audio file through ShaderAudio.ffhook")
        if self.kind == "pipe" or self.container != "avi":
            raise ValueError(f"{rule}: {'a pipe' if self.kind == 'pipe' else repr(self.path.suffix)} delivers the bare {'PNG' if self.png else 'JPEG'} images back to back")
        loaded = [module for module in self.scene.modules if isinstance(module, ShaderAudio) and module._file_reader is not None]
        wanted = self.sound_track
        if wanted is True:
            if len(loaded) > 1:
                raise ValueError(f"sound_track=True: the scene has {len(loaded)} audio modules with a clip ({', '.join(repr(m.name) for m in loaded)}); name one")
            chosen = loaded
        elif isinstance(wanted, str):
            chosen = [module for module in loaded if module.name == wanted][:1]
        else:
            chosen = [module for module in loaded if module is wanted]
        if not chosen:
            which = "no audio module" if wanted is True else f"no audio module {getattr(wanted, 'name', wanted)!r}"
            raise ValueError(f"sound_track: the scene has {which} with a loaded clip (ShaderAudio file= or load(samples=…))")
        reader = chosen[0]._file_reader
        return mjpeg.SoundTrack(reader.samples, reader.samplerate)

    @property
    def wants_opendml(self) -> bool:
        return self.opendml is not None and self.opendml is not False

    def find_budget(self) -> int:
        """The segment size `opendml` asks for; ValueError when the export is no `.avi` file of an mjpeg or png export, or the size is out of range"""
        rule = "opendml goes with an '.avi' file of a Motion-JPEG or PNG export (output='clip.avi', pixel_format='mjpeg' or 'png')"
        if not self.sized:
            raise ValueError(f"{rule}, not pixel_format {self.pixel_format!r}")
        if self.kind == "pipe" or self.container != "avi":
            raise ValueError(f"{rule}: {'a pipe' if self.kind == 'pipe' else repr(self.path.suffix)} delivers the bare {'PNG' if self.png else 'JPEG'} images back to back, without a limit")
        return mjpeg.check_opendml(self.opendml)

    def avi_writer(self, fileno: Optional[int]) -> mjpeg.AviWriter:
        return mjpeg.AviWriter(fileno, self.scene.width, self.scene.height, self.scene.fps, track=self._track,
                               fourcc=b"MPNG" if self.png else b"MJPG", opendml=self._budget)

    def ffmpeg_output(self, output) -> None:
        if self.sized:
            if (output in ("pipe", "-", bytes)):
                self.kind = "pipe"
            else:
                self.path = Path(output).expanduser().absolute()
                self.container = mjpeg.container_of(self.path.suffix, self.pixel_format)
                self.kind = "path-mjpeg"
            if self.wants_track:
                self._track = self.find_track()
            if self.wants_opendml:
                self._budget = self.find_budget()
            if self.path is not None:
                self.path.parent.mkdir(parents=True, exist_ok=True)
            if self.top_down is None:
                self.top_down = False                         # the encoder reads the rows in the order it needs
            return
        if self.wants_track:
            self.find_track()
        if self.wants_opendml:
            self.find_budget()
        if (output in ("pipe", "-", bytes)):
            self.kind = "pipe"
            self.ffmpeg.pipe_output()
        elif ("tcp://" in str(output)):
            raise NotImplementedError
        else:
            self.path = Path(output).expanduser().absolute()
            self.path.parent.mkdir(parents=True, exist_ok=True)
            raw = self.path.suffix.lower() in (".rgb", ".raw", ".rgb24", ".yuv", ".i420")
            self.kind = "path-raw" if (raw or not self.ffmpeg.available()) else "path-ffmpeg"
            if self.kind == "path-raw" and not raw:
                logger.warning(f"No ffmpeg binary on PATH: writing raw rgb24 frames (rows bottom-up) to {self.path}")
            self.ffmpeg.output(path=self.path)
        if self.top_down is None:
            self.top_down = (self.kind == "path-ffmpeg")
        if self.top_down:                                     # the flip happens while the frame is written on the device
            self.ffmpeg.filters = [stage for stage in self.ffmpeg.filters if stage.kind != "vflip"]
            self.ffmpeg.vflip(device=True)

    def ffhook(self) -> None:
        for module in self.scene.modules:
            module.ffhook(self.ffmpeg)

    def popen(self, open_sink: bool = True) -> None:
        """`open_sink=False`: a rank of a sharded export that renders frames but does not own the sink — it still has to write
        its rows in the order the sink wants"""
        self.scene.context.output_top_down(bool(self.top_down))
        if not open_sink:
            return
        if self.kind == "path-ffmpeg":
            # the encoder's own output goes to temporary files, never to a pipe nobody drains (the reference hands ffmpeg
            # file-backed pipes for the same reason, exporting.py:131-132): a chatty encoder cannot stall the export
            self._encoder_log = tempfile.TemporaryFile(mode="w+b")
            self.process = self.ffmpeg.popen(stdin=subprocess.PIPE, stdout=self._encoder_log, stderr=self._encoder_log)
            self.fileno = self.process.stdin.fileno()
        elif self.kind == "path-raw":
            self.file = open(self.path, "wb")
            self.fileno = self.file.fileno()
        elif self.kind == "path-mjpeg":
            self.file = open(self.path, "wb", buffering=0)
            self.fileno = self.file.fileno()
            if self.container == "avi":
                self._avi = self.avi_writer(self.fileno)
                self._avi.begin()
        elif self.kind == "pipe":
            self.file = tempfile.TemporaryFile(mode="w+b")
            self.fileno = self.file.fileno()

    # buffers and piping ---------------------------------------------------------------------------------------

    def make_buffers(self, n: int = 2) -> None:
        self.release_buffers()
        handle = N.Handle()
        if self.sized:
            N.check(N.lib().sfx_ring_create_sized(self.scene.context.handle, self.frame_bytes, max(1, n), 1 if self.container == "avi" else 0, C.byref(handle)))
        else:
            N.check(N.lib().sfx_ring_create(self.scene.context.handle, self.frame_bytes, max(1, n), C.byref(handle)))
        self.ring, self.slots = handle, max(1, n)
        if self._track is not None:
            self._track_ends = self._track.ends(self.total_frames, self.scene.fps)
            N.check(N.lib().sfx_ring_side_track(handle, self._track.pcm.ctypes.data, self._track.pcm.nbytes,
                                                N.as_ptr(self._track_ends, C.c_uint64), len(self._track_ends)))
        if self._budget is not None:                          # (the headers' size is fixed once opendml and the track are known)
            N.check(N.lib().sfx_ring_segments(handle, len(self.avi_writer(None).headers(0, 0, 0, 0)), self._budget, mjpeg.GAP_BYTES))
        if self.staged:
            self._yuv_slots = [self.scene.context.alloc(self.frame_bytes) for _ in range(self.slots)]

    def release_buffers(self) -> None:
        try:
            if self.ring is not None and self.ring.value:
                self.check(N.lib().sfx_ring_pipe_sync(self.ring, -1))
        finally:
            if self.ring is not None and self.ring.value:
                if self.sized:
                    N.lib().sfx_ring_pipe_sync(self.ring, -1)
                    count = C.c_size_t()
                    N.check(N.lib().sfx_ring_sizes(self.ring, None, 0, C.byref(count)))
                    sizes = (C.c_uint32*max(1, count.value))()
                    N.check(N.lib().sfx_ring_sizes(self.ring, sizes, count.value, C.byref(count)))
                    self._sizes += list(sizes[:count.value])
                    N.check(N.lib().sfx_ring_segment_cuts(self.ring, None, 0, C.byref(count)))
                    cuts = (C.c_uint32*max(1, count.value))()
                    N.check(N.lib().sfx_ring_segment_cuts(self.ring, cuts, count.value, C.byref(count)))
                    self._cuts += list(cuts[:count.value])
                N.lib().sfx_ring_destroy(self.ring)
            for pointer in self._yuv_slots:
                self.scene.context.free(pointer)
            self._yuv_slots = []
            self.ring, self.slots = None, 0
            if self._encoder is not None:
                self._encoder.destroy()
                self._encoder = None

    def _check_encoder(self) -> None:
        if (self.process is not None) and (self.process.poll() is not None):
            raise RuntimeError("FFmpeg process closed unexpectedly with traceback:\n" + self.encoder_output())

    def encoder_output(self) -> str:
        """What the encoder process has printed so far (stdout and stderr share one temporary file)"""
        log = getattr(self, "_encoder_log", None)
        if log is None:
            return ""
        log.flush()
        log.seek(0)
        return log.read().decode("utf-8", "replace")

    def pipe(self, turbo: bool = False) -> None:
        """Queue the frame that was just rendered (exporting.py:151-174)"""
        if (self.fileno is None) or (self.ring is None):
            return
        self._check_encoder()
        slot = self.frame % self.slots
        if self.staged:
            # the slot's last frame has left its staging buffer; then convert (on the render stream, in order with the draws) and read out
            self.check(N.lib().sfx_ring_pipe_sync(self.ring, slot))
            self.to_sink(self.scene._final.texture.texture.device_ptr(), self._yuv_slots[slot])
            self.check(N.lib().sfx_ring_read_device_async(self.ring, C.c_void_p(self._yuv_slots[slot]), slot))
        else:
            N.check(N.lib().sfx_ring_read_async(self.ring, self.scene._final.texture.texture.handle, slot))
        N.check(N.lib().sfx_ring_pipe(self.ring, slot, self.fileno))
        if not turbo:
            self.check(N.lib().sfx_ring_pipe_sync(self.ring, slot))

    def fence(self, which: int) -> None:
        """Everything launched on the render stream so far is what frames read against fence `which` depend on"""
        if self.ring is not None:
            N.check(N.lib().sfx_ring_fence(self.ring, which))

    def render_waits_for_last_read(self) -> None:
        """The render stream may not overwrite a frame buffer before the last queued read of it has finished"""
        if self.ring is not None and self.frame > 0:
            N.check(N.lib().sfx_ring_stream_wait(self.ring, (self.frame - 1) % self.slots))

    def drain(self) -> None:
        """Every queued frame has left its device buffer and reached the sink (gathered buffers are reused right after)"""
        if self.ring is not None and self.ring.value:
            self.check(N.lib().sfx_ring_pipe_sync(self.ring, -1))

    def pipe_device(self, device_ptr: int, *, rgb: bool, turbo: bool = True, fence: Optional[int] = None) -> None:
        """Same, for a frame in a raw device buffer: an RGB8 frame (`rgb`, converted here for a planar sink) or a sink frame"""
        if (self.fileno is None) or (self.ring is None):
            return
        self._check_encoder()
        slot = self.frame % self.slots
        if rgb and self.staged:
            self.check(N.lib().sfx_ring_pipe_sync(self.ring, slot))
            self.to_sink(device_ptr, self._yuv_slots[slot])
            device_ptr, fence = self._yuv_slots[slot], None
        if fence is None:
            self.check(N.lib().sfx_ring_read_device_async(self.ring, C.c_void_p(device_ptr), slot))
        else:
            self.check(N.lib().sfx_ring_read_fenced_async(self.ring, C.c_void_p(device_ptr), slot, fence))
        N.check(N.lib().sfx_ring_pipe(self.ring, slot, self.fileno))
        if not turbo:
            self.check(N.lib().sfx_ring_pipe_sync(self.ring, slot))

    def pipe_device_frames(self, device_ptr: int, stride: int, count: int, turbo: bool = True, fence: Optional[int] = None) -> None:
        """`count` consecutive SINK frames of a batch in one native call (the per-frame python loop costs more than the frames themselves
        when they are small); with a progress relay, or without turbo, frame by frame as before"""
        if self.relay is not None or not turbo or self.fileno is None or self.ring is None:
            for i in range(count):
                self.pipe_device(device_ptr + i*stride, rgb=False, turbo=turbo, fence=fence)
                self.update()
            return
        self._check_encoder()
        self.check(N.lib().sfx_ring_pipe_frames(self.ring, C.c_void_p(device_ptr), stride, count, self.frame % self.slots, -1 if fence is None else fence, self.fileno))
        self.frame += count

    # finish ---------------------------------------------------------------------------------------------------------

    def finish(self):
        output = None
        self.scene.context.synchronize()
        try:
            self.release_buffers()
        except BaseException:
            if self.file is not None:                         # (an mjpeg frame that did not fit: the sink is closed as far as it got)
                self.file.close()
            raise
        finally:
            self.scene.context.output_top_down(False)
        if self.kind == "path-mjpeg":
            output = self.path
            if self.file is not None:
                try:
                    if self._avi is not None:
                        self._avi.finish(self._sizes)
                finally:
                    self.file.close()
        elif self.process is not None:
            self.process.stdin.close()
            if self.process.wait() != 0:                      # the reference only waits (exporting.py:186-187); say what went wrong
                logger.error(f"FFmpeg exited with status {self.process.returncode}:\n" + self.encoder_output())
            output = self.path
        elif self.kind == "path-ffmpeg":
            output = self.path                                # a rank that does not own the sink
        elif self.kind == "path-raw":
            if self.file is not None:
                self.file.close()
            output = self.path
        elif self.kind == "pipe" and self.file is not None:
            self.file.seek(0)
            output = self.file.read()
            self.file.close()
        self.took = (time.monotonic() - self.start)
        self.log_stats(output)
        return output

    def log_stats(self, output) -> None:
        took = self.took or 1e-9
        logger.info(f"Finished rendering ({output if not isinstance(output, bytes) else f'{len(output)} bytes'}) • "
                    f"took {took:.2f}s at {self.frame/took:.2f} fps | {self.scene.runtime/took:.2f}x realtime, {self.frame} frames")


class SinkBatches:
    """`count` device buffers of `batch` sink frames, and the rule that fills them: a batch is rendered straight into place as rgb24, or
    into one RGB8 scratch of a batch and converted right behind as yuv420p, mjpeg or png — both on the context's stream, so one scratch serves every
    buffer (allocated by the first batch rendered through it)."""

    def __init__(self, export: ExportingHelper, batch: int, count: int = 2):
        self.export, self.batch, self.context = export, batch, export.scene.context
        self.rgb_bytes = export.scene.width*export.scene.height*3
        self.scratch: Optional[int] = None
        self.last_rgb: Optional[int] = None                 # the last RGB8 frame of the last batch rendered (for iFinal)
        self.buffers = [self.context.alloc(export.frame_bytes*batch) for _ in range(count)]

    def render(self, target: int, count: int, draw: Callable[[int, int], None]) -> None:
        """`draw(count, pointer)` renders `count` RGB8 frames at `pointer`; they end up as sink frames at `target`"""
        assert 0 < count <= self.batch, (count, self.batch)
        rgb = target
        if self.export.staged:
            if self.scratch is None:
                self.scratch = self.context.alloc(self.rgb_bytes*self.batch)
            rgb = self.scratch
        draw(count, rgb)
        if rgb != target:
            self.export.to_sink(rgb, target, count)
        self.last_rgb = rgb + (count - 1)*self.rgb_bytes

    def close(self) -> None:
        self.context.synchronize()
        for pointer in self.buffers + ([self.scratch] if self.scratch is not None else []):
            self.context.free(pointer)
        self.buffers, self.scratch = [], None
