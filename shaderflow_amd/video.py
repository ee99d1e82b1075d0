"""
ShaderVideo: a video as a texture, one new frame whenever scene time passes the next frame's timestamp.

Host mirror of the reference's shaderflow/video.py:13-66 — same fields (`name, path, texture, width, height, fps`),
same texture (RGB8, `iVideo`, size of the content; set `.texture.temporal` for frame history) and the same update
rule: a frame is uploaded only when `scene.time > frames_read/fps` (so nothing is uploaded on the first scene
frame), rows flipped to GL order, after rolling the temporal matrix.

Where frames come from: the reference pipes the file through an `ffmpeg` subprocess (ffmpeg.py:1116-1137). Here:
  * `frames=` any iterable of (height, width, 3) uint8 arrays, top row first — what that iterator yields; with `format="i420"` the
    iterable yields 1-D uint8 arrays of width*height*3//2 bytes instead (planar 4:2:0: Y, U, V, top row first); with a planar pixel
    format ("yuv420p", "yuv422p", "yuv444p", each also with "10le" or "12le", or "gray") 1-D uint8 arrays of that layout's frame
    size, or uint16 arrays of the samples for the deep layouts;
  * `path=` a `.npy` holding (n, height, width, 3) uint8, or a raw `.rgb` file with `width`/`height` given;
  * `path=` a `.y4m` file (YUV4MPEG2, the uncompressed interchange format: 1.5 bytes per pixel), read natively: width, height and
    fps come from its header, and so does the layout (planarsource.py): progressive 4:2:0 (`C420`, `C420jpeg`, `C420mpeg2`,
    `C420paldv`, or no `C` tag), 4:2:2 (`C422`), 4:4:4 (`C444`), each at 8, 10 or 12 bits (`p10`, `p12`), grey (`Cmono`), limited
    or full range (`XCOLORRANGE=`). Interlacing, alpha, `C411`, other depths and deep grey raise ValueError naming the tag;
  * `path=` a raw `.yuv` / `.i420` file with `width`, `height` and `fps` given: planar frames of `format` (yuv420p when none is
    given: what this package's own yuv420p export writes, exporting.py — with `yuv_matrix="bt709"` when the export had it);
  * `path=` an `.avi` file with a Motion-JPEG video stream (fourcc `MJPG`: what `pixel_format="mjpeg"` exports, and what many cameras
    and editors write) or a bare `.mjpeg` / `.mjpg` stream (JPEG images back to back; `fps=` given), read natively (mjpegsource.py):
    the frames stay compressed in pinned memory and over the link — a quality-90 4K frame is about 665 KB against 24.9 MB of rgb24 —
    and are decoded on the device into the texture (csrc/jpeg_decode_kernels.hpp: baseline, 8 bit, one interleaved scan, 4:2:0 /
    4:2:2 / 4:4:4 / grey; anything else raises ValueError naming the marker or field). With `format="mjpeg"`, `frames=` yields such
    streams as `bytes`. A frame whose entropy-coded data is damaged raises RuntimeError naming the source frame; it is not drawn. A
    stream without restart markers is cut into subsequences that decode in parallel: entropy decoding on the host is out of scope.
    An `.avi` that continues in OpenDML `RIFF 'AVIX'` segments (what `opendml=` exports, and large captures: files past 4 GiB) is read to
    its end, for this codec and the next (clips.py);
  * `path=` an `.avi` file with a PNG video stream (fourcc `MPNG`: what `pixel_format="png"` exports), read natively (pngsource.py): the
    PNG files stay compressed in pinned memory and over the link and are inflated and unfiltered on the device into the texture,
    bit-exactly (csrc/png_decode_kernels.hpp: 8-bit RGB without interlace; anything else raises ValueError naming the IHDR field; chunk
    CRC-32s are not checked, the Adler-32 is, on the device). With `format="png"`, `frames=` yields PNG files as `bytes` — numbered
    files are `frames=(p.read_bytes() for p in sorted(folder.glob("*.png")))`. A damaged frame raises RuntimeError naming the source
    frame; it is not drawn;
  * any other `path` (an `.avi` with another codec included) is decoded by an `ffmpeg` binary on PATH when there is one (rawvideo rgb24 over a pipe),
    otherwise construction raises — there is no silent fallback.
A source shorter than the scene keeps its last frame on screen (the reference's generator would raise
StopIteration out of `update`).

Planar sources are converted on the device (csrc/video_kernels.hpp, whose header comment is the definition): integer arithmetic with
the layout's matrix (`yuv_matrix`: bt601, bt709, bt2020), range (`yuv_range`) and depth, subsampled chroma replicated
(`chroma="nearest"`) or interpolated with the triangle filter at the file's siting (`chroma="linear"`) — this project's own
definition, **unpinned against swscale** (no ffmpeg binary to pin it against), like the yuv420p output. The 8-bit 4:2:0 bt601 limited
nearest layout is `format == "i420"` and `k_video_frame`'s, as ever; every other one is `format == "planar"` (the layout in `header`)
and `k_video_planar`'s, which gives the same bytes at that layout. The frame loop shows them through the same kernels (`VideoStage`:
a pinned frame, an asynchronous copy, one launch), so the conversion has one definition; rgb sources in the frame loop are flipped and
uploaded by the host as ever.
Scenes that qualify draw whole chunks of frames per native call instead (videosequence.py).
"""
from __future__ import annotations

import ctypes as C
import shutil
import subprocess
from collections.abc import Iterable, Iterator
from pathlib import Path
from typing import Optional

import numpy as np
from attrs import define

from shaderflow_amd import _native as N
from shaderflow_amd import mjpegsource, planarsource, pngsource
from shaderflow_amd.clips import AviClip
from shaderflow_amd.module import ShaderModule, logger
from shaderflow_amd.texture import ShaderTexture

CODECS = {"mjpeg": mjpegsource, "png": pngsource}                    # a compressed `format` → the module that reads, stages and decodes it
MJPEG_SUFFIXES = (".mjpeg", ".mjpg")
Y4M_CHROMA = ("420", "420jpeg", "420mpeg2", "420paldv")              # all read as the same 8-bit 4:2:0 bytes (the siting is not interpolated)
PLANAR_SUFFIXES = (".yuv", ".i420")                                   # raw planar frames: the suffixes exporting.py's yuv420p sink writes


def _probe(path: Path) -> tuple[int, int, float]:
    """(width, height, fps) of a video file through ffprobe"""
    out = subprocess.check_output(["ffprobe", "-v", "error", "-select_streams", "v:0", "-show_entries",
                                   "stream=width,height,r_frame_rate", "-of", "csv=p=0", str(path)], text=True).strip()
    width, height, rate = out.split(",")[:3]
    num, _, den = rate.partition("/")
    return int(width), int(height), float(num)/float(den or 1)


def iter_video_frames(path: Path, width: int, height: int) -> Iterator[np.ndarray]:
    """(height, width, 3) uint8 frames of `path`, top row first, decoded by an ffmpeg subprocess"""
    process = subprocess.Popen(["ffmpeg", "-hide_banner", "-loglevel", "error", "-i", str(path), "-f", "rawvideo",
                                "-pix_fmt", "rgb24", "-"], stdout=subprocess.PIPE)
    size = width*height*3
    try:
        while len(raw := process.stdout.read(size)) == size:
            yield np.frombuffer(raw, np.uint8).reshape(height, width, 3)
    finally:
        process.kill()


def parse_y4m_header(line: bytes) -> tuple[int, int, float]:
    """(width, height, fps) of a YUV4MPEG2 stream header: the 8-bit 4:2:0 limited-range front of planarsource.parse_y4m. ValueError
    names the tag this reader does not take"""
    width, height, fps, fields = planarsource.parse_y4m(line)
    if fields["subsampling"] != "420" or fields["depth"] != 8:
        raise ValueError(f"y4m tag {fields['tags']['C']!r}: only 8-bit 4:2:0 ({', '.join('C' + c for c in Y4M_CHROMA)}) is read")
    if fields["range"] == "full":
        raise ValueError(f"y4m tag {fields['tags']['X']!r}: only limited-range video is read")
    return width, height, fps


class PlanarFile(planarsource.PlanarReader):
    """Frames of an 8-bit 4:2:0 `.y4m` or raw planar file, in order: an iterator of 1-D uint8 arrays of width*height*3//2 bytes, and
    `readinto(view)` (planarsource.PlanarReader: the frame loop every planar reader shares). Another layout raises ValueError naming
    the tag: `planarsource.PlanarClip`, which ShaderVideo opens, reads those."""

    def _header(self, line: bytes) -> tuple[int, int, float]:
        return parse_y4m_header(line)

    def _frame_bytes(self) -> int:
        return self.width*self.height*3//2


class VideoStage:
    """sfx_video_* (include/shaderflow_hip.h) for one ShaderVideo: `slots` pinned frames the host fills (`view`), their asynchronous
    copies (`submit`) and k_video_frame into the texture matrix (`step`, or a landing frame of the native sequence). The handle holds
    the matrix' boxes in their order at creation and rolls with every frame it lands: the host rolls its ShaderTexture alike."""

    def __init__(self, video: "ShaderVideo", slots):
        """`slots`: how many, or a function that says it from `frame_bytes` (videosequence.slot_count)"""
        texture = video.texture
        if texture.layers != 1 or texture.components != 3 or texture.dtype != np.uint8:
            raise ValueError("a staged video needs an RGB8 texture with layers = 1")
        boxes = [box.texture for (_, _, box) in texture.boxes]
        self.serials = tuple(box.serial for box in boxes)              # which device textures the handle writes into
        self.planar, self.codec = video.format in ("i420", "planar"), CODECS.get(video.format)      # planar: 1-D frames of a fixed size
        self.layout = video.header if video.format == "planar" else None                           # a planarsource.PlanarLayout: k_video_planar's
        self.width, self.height, self.header = video.width, video.height, video.header
        if self.codec:
            self.frame_bytes = video.capacity                         # what a slot holds
        elif self.layout:
            self.frame_bytes = self.layout.frame_bytes(video.width, video.height)
        else:
            self.frame_bytes = video.width*video.height*3//(2 if self.planar else 1)
        self.slots, self.handle = slots(self.frame_bytes) if callable(slots) else slots, N.Handle()
        handles = (N.Handle*len(boxes))(*[box.handle for box in boxes])
        if self.codec:
            self.handle = self.codec.create(video.scene.context.handle, handles, texture.temporal, video.header, video.capacity, self.slots)
            return
        if self.layout:
            native = self.layout.native()
            N.check(N.lib().sfx_video_create_planar(video.scene.context.handle, handles, texture.temporal, video.width, video.height,
                                                    C.byref(native), self.slots, C.byref(self.handle)))
            return
        N.check(N.lib().sfx_video_create(video.scene.context.handle, handles, texture.temporal, video.width, video.height,
                                         N.VIDEO_I420 if self.planar else N.VIDEO_RGB24, self.slots, C.byref(self.handle)))

    def view(self, slot: int) -> np.ndarray:
        """The slot's pinned frame as a 1-D uint8 array (waits until the frame it held before has been consumed)"""
        pointer, nbytes = C.c_void_p(), C.c_size_t()
        N.check(N.lib().sfx_video_slot(self.handle, slot, C.byref(pointer), C.byref(nbytes)))
        return np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint8)), shape=(nbytes.value,))

    def fill(self, view: np.ndarray, frame, label: str) -> Optional[int]:
        """One source frame — an rgb array, an i420 array, a planar array of the layout or a JPEG stream, as the video's format says —
        into the pinned `view`; returns the bytes to `submit` (None: the format's fixed size). `label` names the frame in an error."""
        if self.codec:                                                # the stream's tables, interval starts and scan (a PNG file's IDAT data); only they are copied
            return self.codec.stage(frame, self.header, view, label)
        if self.layout and self.layout.depth > 8 and getattr(frame, "dtype", None) == np.uint16:
            frame = np.ascontiguousarray(frame).astype("<u2", copy=False).reshape(-1).view(np.uint8)     # deep samples: little-endian words
        frame = np.asarray(frame, np.uint8)
        if frame.size != self.frame_bytes:
            kind = f"a planar {self.layout.describe()}" if self.layout else ("an i420" if self.planar else "an rgb")
            raise ValueError(f"{label}: {kind} frame of {self.width} x {self.height} has {self.frame_bytes} bytes, the source gave {frame.size}")
        np.copyto(view.reshape(frame.shape), frame)                   # (a memory-mapped clip is read here, without the GIL)
        return None

    def put_back(self, held):
        """What goes back in front of the source for a frame that was taken from it and not drawn: `held` is the stream a compressed
        frame came as, or the pinned view an uncompressed one was copied into — a copy of it, shaped as the source yields frames"""
        return held if self.codec else held.copy().reshape((-1,) if self.planar else (self.height, self.width, 3))

    def submit(self, slot: int, nbytes: Optional[int] = None) -> None:
        """`nbytes`: the bytes the frame has (a compressed frame: only they are copied)"""
        if nbytes is None:
            N.check(N.lib().sfx_video_submit(self.handle, slot))
        else:
            N.check(N.lib().sfx_video_submit_bytes(self.handle, slot, nbytes))

    def bad_frame(self, wait: bool = False) -> Optional[tuple[int, int]]:
        """(how many frames the stage had landed before it, status) of the first landed frame since the last call whose compressed data
        was bad — it was not drawn; None when there is none. `wait`: for everything queued on the context's stream first."""
        frame, status = C.c_int64(-1), C.c_uint32(0)
        N.check(N.lib().sfx_video_status(self.handle, 1 if wait else 0, C.byref(frame), C.byref(status)))
        return None if frame.value < 0 else (frame.value, status.value)

    def paths(self) -> tuple[int, int]:
        """Landed compressed frames by the codec's two decode paths: (the parallel one, the serial one) — Motion-JPEG: a lane per
        subsequence / per restart interval; PNG: a wave per segment / one wave for the stream, chosen so or fallen back to"""
        return self.codec.paths(self.handle)

    def describe_status(self, status: int) -> str:
        return self.codec.describe_status(status)

    def step(self, slot: int) -> None:
        N.check(N.lib().sfx_video_step(self.handle, slot))

    def release(self) -> None:
        if self.handle is not None and self.handle.value:
            N.lib().sfx_video_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


@define(eq=False, slots=False)
class ShaderVideo(ShaderModule):
    name: str = "iVideo"
    path: Optional[Path] = None
    frames: Optional[Iterable] = None
    texture: ShaderTexture = None
    width: Optional[int] = None
    height: Optional[int] = None
    fps: Optional[float] = None
    format: Optional[str] = None
    """None: the source yields rgb arrays; "i420": planar 4:2:0 frames of width*height*3//2 bytes (set by the planar file sources);
    "mjpeg": baseline JPEG streams as `bytes` (set by the Motion-JPEG file sources); "png": PNG files as `bytes` (set by an MPNG `.avi`).
    A planar pixel format may be given for a raw `.yuv` file or for `frames=`: "yuv420p", "yuv422p", "yuv444p" (each also with "10le"
    or "12le") or "gray". Once the source is open the field reads "i420" when the layout is 8-bit 4:2:0 bt601 limited nearest, and
    "planar" — the layout in `header` — for every other one."""
    header: Optional[object] = None
    """format "mjpeg" / "png": the first frame's header (mjpegsource.JpegHeader / pngsource.PngHeader): the geometry every frame must
    have; format "planar": the frames' planarsource.PlanarLayout"""
    yuv_matrix: str = "bt601"
    """planar sources: "bt601", "bt709" (what `ExportingHelper.yuv_matrix = "bt709"` exports) or "bt2020" — no file says it"""
    yuv_range: Optional[str] = None
    """planar sources: "limited" or "full"; None: a `.y4m` file's XCOLORRANGE tag, else limited"""
    chroma: str = "nearest"
    """planar sources: subsampled chroma replicated ("nearest") or interpolated ("linear": the triangle filter, sited as the file says)"""
    capacity: int = 0
    """format "mjpeg" / "png": bytes of a staged frame at the most (from the container's largest chunk; for `frames=` a raw picture's worth)"""
    _stage: Optional[VideoStage] = None
    _clip: Optional[object] = None
    _reader: Optional[Iterator] = None
    _read: int = 0
    _exhausted: bool = False

    def __attrs_post_init__(self):
        ShaderModule.__attrs_post_init__(self)
        if self.format not in (None, "i420", *CODECS, *planarsource.FORMAT_NAMES):
            raise ValueError(f"ShaderVideo format {self.format!r}: None (rgb arrays), 'i420', 'mjpeg', 'png' or a planar pixel format ({', '.join(planarsource.FORMAT_NAMES)})")
        self._reader = self._open()
        if not all((self.width, self.height, self.fps)):
            raise ValueError("ShaderVideo needs width, height and fps (give them, or a source they can be read from)")
        if self.format == "i420" and (self.width % 2 or self.height % 2):
            raise ValueError(f"a 4:2:0 source needs even extents, not {self.width} x {self.height}")
        if self.format == "planar":
            self.header.check_extents(self.width, self.height)
        self.texture = ShaderTexture(scene=self.scene, name=self.name, width=self.width, height=self.height,
                                     dtype=np.uint8, components=3)

    def _open(self) -> Iterator[np.ndarray]:
        if self.frames is not None:
            if isinstance(self.frames, np.ndarray) and self.format is None:
                self.height, self.width = self.height or self.frames.shape[1], self.width or self.frames.shape[2]
            if self.format in CODECS:
                return self._open_compressed(iter(self.frames), None)
            if self.format is not None:                                 # 1-D planar frames (uint16 arrays for the deep layouts)
                self._take_layout(planarsource.PlanarLayout.from_format(self.format, matrix=self.yuv_matrix, range=self.yuv_range or "limited", chroma=self.chroma))
            return iter(self.frames)
        if self.path is None:
            raise ValueError("ShaderVideo needs `path=` or `frames=`")
        self.path = Path(self.path)
        suffix = self.path.suffix.lower()
        if suffix == ".npy":
            clip = np.load(self.path, mmap_mode="r")
            self.height, self.width = self.height or clip.shape[1], self.width or clip.shape[2]
            return iter(clip)
        if suffix in (".rgb", ".raw", ".rgb24"):
            if not all((self.width, self.height)):
                raise ValueError("raw rgb24 video needs width= and height=")
            clip = np.memmap(self.path, np.uint8, "r").reshape(-1, self.height, self.width, 3)
            return iter(clip)
        if suffix == ".y4m" or suffix in PLANAR_SUFFIXES:
            if suffix != ".y4m" and not all((self.width, self.height, self.fps)):
                raise ValueError("raw planar yuv420p video needs width=, height= and fps=")
            if self.format in CODECS:
                raise ValueError(f"{self.path}: a planar file is not format {self.format!r}")
            clip = planarsource.PlanarClip(self.path, self.width, self.height, self.fps, format=self.format, matrix=self.yuv_matrix,
                                           range=self.yuv_range, chroma=self.chroma)
            self.width, self.height, self.fps = clip.width, clip.height, self.fps or clip.fps
            self._take_layout(clip.layout)
            return clip
        if suffix in MJPEG_SUFFIXES:
            self._clip = clip = mjpegsource.RawReader(self.path, self.fps)
            return self._open_compressed(clip, clip.largest)
        if suffix == ".avi":
            try:
                clip = AviClip(self.path, CODECS.values())
            except LookupError:                                       # an AVI file with another codec: ffmpeg's, as before
                pass
            else:
                self._clip, self.fps, self.format = clip, self.fps or clip.fps, clip.format
                return self._open_compressed(clip, clip.largest)
        if not (shutil.which("ffmpeg") and shutil.which("ffprobe")):
            raise RuntimeError(f"{self.path}: decoding this container needs the ffmpeg and ffprobe binaries; "
                               "give frames=, a .npy clip or a raw .rgb file instead")
        width, height, fps = _probe(self.path)
        self.width, self.height, self.fps = self.width or width, self.height or height, self.fps or fps
        return iter_video_frames(self.path, self.width, self.height)

    def _take_layout(self, layout: "planarsource.PlanarLayout") -> None:
        """The two paths of a planar source: the I420 layout keeps k_video_frame and its bytes, every other one is k_video_planar's"""
        self.format, self.header = ("i420", None) if layout.is_i420 else ("planar", layout)

    def _open_compressed(self, source: Iterator, largest: Optional[int]) -> Iterator:
        """A source of JPEG streams, or of PNG files (`format`): the clip's geometry and sampling are its first frame's"""
        import itertools
        self.format = self.format or "mjpeg"
        codec = CODECS[self.format]
        first = next(source, None)
        if first is None:
            raise ValueError(f"{self.name}: a {codec.TITLE} source without a frame")
        self.header = codec.parse_header(first)
        if (self.width and self.width != self.header.width) or (self.height and self.height != self.header.height):
            raise ValueError(f"{self.name}: the frames are {self.header.width} x {self.header.height}, not {self.width} x {self.height}")
        self.width, self.height = self.header.width, self.header.height
        self.capacity = codec.capacity_for(self.header, largest)
        return itertools.chain([first], source)

    def update(self) -> None:
        if self._exhausted or not (self.scene.time > (self._read/self.fps)):       # video.py:60
            return
        try:
            frame = next(self._reader)
        except StopIteration:
            self._exhausted = True
            logger.warning(f"{self.name}: source ended after {self._read} frames, holding the last one")
            return
        if self.format in CODECS:
            self._read += 1                                             # (a damaged frame is passed over: the next update() shows the next one)
            self._show_staged(frame, self._read - 1)
            return
        if self.format in ("i420", "planar"):
            self._show_staged(frame, self._read)
        else:
            frame = np.ascontiguousarray(np.flip(np.asarray(frame, np.uint8), axis=0))
            self.texture.roll()
            self.texture.write(frame)
        self._read += 1

    def _show_staged(self, frame, source: int) -> None:
        """A planar frame through k_video_frame, a compressed one through the decode kernels — the one definition of either: a pinned
        slot, its copy, the launch"""
        boxes = tuple(box.texture.serial for (_, _, box) in self.texture.boxes)
        if self._stage is not None and self._stage.serials != boxes:      # the texture was re-made, or rolled by somebody else
            self._stage.release()
            self._stage = None
        if self._stage is None:
            self._stage = VideoStage(self, slots=1)
        stage = self._stage
        stage.submit(0, stage.fill(stage.view(0), frame, f"{self.name}: source frame {source}"))
        stage.step(0)
        bad = stage.bad_frame(wait=True)                              # (only a compressed frame can be bad: nothing is waited for otherwise)
        self.texture.roll()                                           # (the device rolled its matrix even when it left a bad frame's box alone)
        stage.serials = tuple(box.texture.serial for (_, _, box) in self.texture.boxes)
        if bad is not None:
            raise RuntimeError(f"{self.name}: source frame {source} could not be decoded: {stage.describe_status(bad[1])}")
        self.texture.refresh_host_copy()

    def destroy(self) -> None:
        if self._stage is not None:
            self._stage.release()
            self._stage = None
        if self._clip is not None:                                     # a Motion-JPEG file's map
            self._clip.close()
            self._clip = None
