"""
General planar sources on the device (csrc/video_kernels.hpp k_video_planar, csrc/capi_video.hip sfx_video_create_planar,
shaderflow_amd/planarsource.py, ShaderVideo's `yuv_matrix`, `yuv_range`, `chroma` and planar `format`s):

  1. the kernel through sfx_video_create_planar, sfx_video_step and sfx_texture_read against tests/planar_ref.py's restatement of
     the definition, bit for bit: every subsampling x depth, both filters and both sitings, the matrices and ranges rotated so that
     each occurs with each depth; sizes of one run, a run and a 2-pixel tail, an unaligned pitch, a long row; at the I420 layout the
     existing I420 kernel's bytes;
  2. scenes: the video sequence's export equals the frame loop's byte for byte for a C444 and a C422p10 `.y4m` and a raw bt709 file,
     and the texture is the restatement of the source frame;
  3. the project reads its own bt709 yuv420p export: the texture is the restatement of the exported planes, and closer to the
     rendered picture than a bt601 reading of the same file;
  4. refusals by return code or exception.
"""
from __future__ import annotations

import ctypes as C
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import planar_ref as R                                                 # noqa: E402

pytestmark = pytest.mark.gpu

FPS = 60.0
W, H = 96, 54
CW, CH = 32, 18                                                        # the clips' extents


def layout_of(**fields):
    from shaderflow_amd.planarsource import PlanarLayout
    return PlanarLayout(**fields)


class Stage:
    """sfx_video_* over one bare RGB8 texture of the default context: a planar handle of `layout`, or (`layout` None) the I420 one"""

    def __init__(self, w, h, layout):
        from shaderflow_amd import _native as N
        self.N, self.lib, self.w, self.h = N, N.lib(), w, h
        self.context = N.default_context()
        self.texture, self.handle = N.Handle(), N.Handle()
        N.check(self.lib.sfx_texture_create(self.context.handle, w, h, 3, N.U8, C.byref(self.texture)))
        boxes = (N.Handle*1)(self.texture)
        if layout is None:
            code = self.lib.sfx_video_create(self.context.handle, boxes, 1, w, h, N.VIDEO_I420, 1, C.byref(self.handle))
        else:
            native = layout.native()
            code = self.lib.sfx_video_create_planar(self.context.handle, boxes, 1, w, h, C.byref(native), 1, C.byref(self.handle))
        if code != N.OK:
            self.lib.sfx_texture_destroy(self.texture)
            N.check(code)

    def show(self, frame):
        pointer, nbytes = C.c_void_p(), C.c_size_t()
        self.N.check(self.lib.sfx_video_slot(self.handle, 0, C.byref(pointer), C.byref(nbytes)))
        view = np.ctypeslib.as_array(C.cast(pointer, C.POINTER(C.c_uint8)), shape=(nbytes.value,))
        raw = np.ascontiguousarray(frame).reshape(-1).view(np.uint8)
        assert raw.size == nbytes.value, (raw.size, nbytes.value)
        np.copyto(view, raw)
        self.N.check(self.lib.sfx_video_submit(self.handle, 0))
        self.N.check(self.lib.sfx_video_step(self.handle, 0))
        out = np.empty((self.h, self.w, 3), np.uint8)
        self.N.check(self.lib.sfx_texture_read(self.texture, out.ctypes.data, out.nbytes))
        return np.flipud(out)                                          # top row first, as the restatement

    def close(self):
        self.lib.sfx_video_destroy(self.handle)
        self.lib.sfx_texture_destroy(self.texture)


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------------

def frames_for(layout, w, h, seed):
    """Two random frames, the eight corner triples, random luma over extreme chroma either way, and — deep layouts — words above 2^b - 1"""
    rng, top = np.random.default_rng(seed), 2**layout.depth - 1
    dtype = np.uint16 if layout.depth > 8 else np.uint8
    cw, ch = R.chroma_extents(layout, w, h)
    n, q = w*h, cw*ch
    random = lambda high: rng.integers(0, high + 1, n + 2*q).astype(dtype)                     # noqa: E731
    frames = [random(top), random(top)]
    for luma, cb, cr in itertools.product((0, top), repeat=3):
        frames.append(np.concatenate([np.full(n, luma, dtype), np.full(q, cb, dtype), np.full(q, cr, dtype)]))
    for cb, cr in ((top, 0), (0, top)):
        mixed = random(top)
        mixed[n:n + q], mixed[n + q:] = cb, cr
        frames.append(mixed)
    if layout.depth > 8:
        frames.append(random(65535))
        frames.append(np.full(n + 2*q, 65535, dtype))
    return frames


SUBSAMPLED_SIZES = [(2, 2), (16, 2), (18, 4), (34, 6), (66, 38), (1918, 2)]
SIZES = {"420": SUBSAMPLED_SIZES, "422": SUBSAMPLED_SIZES + [(2, 1), (18, 3)], "444": SUBSAMPLED_SIZES + [(1, 1), (17, 3), (33, 5)],
         "mono": SUBSAMPLED_SIZES + [(1, 1), (17, 3), (33, 5)]}
FILTERS = {"420": [("nearest", "centre"), ("linear", "centre"), ("linear", "left")], "422": [("nearest", "left"), ("linear", "centre"), ("linear", "left")],
           "444": [("nearest", "centre"), ("linear", "left")], "mono": [("nearest", "centre"), ("linear", "centre")]}
COLOURS = list(itertools.product(("bt601", "bt709", "bt2020"), ("limited", "full")))


def kernel_cases():
    """Every subsampling x depth x filter; the six matrix x range pairs rotate through each depth's eight cases, so each pair occurs with
    each depth (and grey, 8 bit only, takes two more)"""
    cases = []
    for depth in (8, 10, 12):
        turn = 0
        for subsampling in ("420", "422", "444") + (("mono",) if depth == 8 else ()):
            for chroma, siting in FILTERS[subsampling]:
                matrix, range_ = COLOURS[(turn + depth) % len(COLOURS)]
                turn += 1
                cases.append(dict(subsampling=subsampling, depth=depth, matrix=matrix, range=range_, chroma=chroma, siting=siting))
    return cases


def case_id(case):
    return "-".join(str(case[key]) for key in ("subsampling", "depth", "matrix", "range", "chroma", "siting"))


def test_the_cases_cover_every_colour_at_every_depth():
    cases = kernel_cases()
    for depth in (8, 10, 12):
        assert {(c["matrix"], c["range"]) for c in cases if c["depth"] == depth} == set(COLOURS)
        assert {(c["subsampling"], c["chroma"], c["siting"]) for c in cases if c["depth"] == depth} >= \
               {(s, f, t) for s in ("420", "422", "444") for f, t in FILTERS[s]}


def check_against_the_restatement(layout, w, h, seed):
    stage = Stage(w, h, layout)
    try:
        clipped = 0
        for k, frame in enumerate(frames_for(layout, w, h, seed)):
            want = R.to_rgb(frame, w, h, layout)
            got = stage.show(frame)
            assert np.array_equal(got, want), (layout.describe(), w, h, k, np.argwhere(got != want)[:4].tolist())
            clipped += int(((want == 0) | (want == 255)).sum())
        assert clipped > 0                                             # the clipping was exercised
    finally:
        stage.close()


@pytest.mark.parametrize("case", kernel_cases(), ids=case_id)
def test_the_kernel_is_the_restatement(case):
    layout = layout_of(**case)
    for w, h in SIZES[case["subsampling"]]:
        check_against_the_restatement(layout, w, h, seed=w*131 + h)


def test_a_full_hd_frame_of_420p10_linear_left():
    check_against_the_restatement(layout_of(subsampling="420", depth=10, matrix="bt709", chroma="linear", siting="left"), 1920, 1080, seed=9)


@pytest.mark.parametrize("w, h", [(2, 2), (16, 2), (18, 4), (66, 38), (1918, 2), (64, 36)])
def test_the_i420_layout_gives_the_i420_kernels_bytes(w, h):
    layout = layout_of()                                               # 8-bit 4:2:0 bt601 limited nearest
    assert layout.is_i420
    general, special = Stage(w, h, layout), Stage(w, h, None)
    try:
        for frame in frames_for(layout, w, h, seed=w + h):
            assert np.array_equal(general.show(frame), special.show(frame))
    finally:
        general.close()
        special.close()


# ---- 2. scenes --------------------------------------------------------------------------------------------------------------------------

def video_scene(source):
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo

    class VideoScene(ShaderScene):
        def build(self):
            self.video = ShaderVideo(scene=self, **source())
            self.shader.fragment = "video"
    return VideoScene


def bare_scene():
    """An initialised scene to hang a ShaderVideo on, for update() frame by frame"""
    from shaderflow_amd.scene import ShaderScene
    scene = ShaderScene()
    scene.initialize()
    return scene


def render(scene, frames):
    raw = scene.main(width=W, height=H, fps=FPS, time=frames/FPS, output=bytes)
    assert len(raw) == frames*W*H*3
    return np.frombuffer(raw, np.uint8).reshape(frames, W*H*3)


def clip_files(tmp_path, count):
    """name → (ShaderVideo's keyword arguments, the layout its frames have, the frames)"""
    out = {}
    for name, header, layout, fields in (
            ("c444", "C444", layout_of(subsampling="444"), {}),
            ("c422p10-linear", "C422p10 XCOLORRANGE=FULL", layout_of(subsampling="422", depth=10, range="full", chroma="linear", siting="left"), dict(chroma="linear")),
            ("raw-bt709", None, layout_of(matrix="bt709"), dict(yuv_matrix="bt709", width=CW, height=CH, fps=30.0))):
        rng = np.random.default_rng(len(name))
        samples = R.frame_bytes(layout, CW, CH)//layout.sample_bytes
        frames = rng.integers(0, 2**layout.depth, (count, samples)).astype("<u2" if layout.depth > 8 else np.uint8)
        path = tmp_path/(name + (".y4m" if header else ".yuv"))
        with open(path, "wb") as file:
            if header:
                file.write(f"YUV4MPEG2 W{CW} H{CH} F30:1 Ip {header}\n".encode())
            for frame in frames:
                file.write((b"FRAME\n" if header else b"") + frame.tobytes())
        out[name] = (dict(path=path, **fields), layout, frames)
    return out


@pytest.mark.parametrize("name", ["c444", "c422p10-linear", "raw-bt709"])
def test_the_video_sequence_gives_the_frame_loops_bytes(name, monkeypatch, tmp_path):
    arguments, layout, frames = clip_files(tmp_path, 30)[name]
    Scene, count = video_scene(lambda: dict(arguments)), 40
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "0")
    loop = Scene()
    want = render(loop, count)
    assert loop.video_sequence is None
    monkeypatch.setenv("SHADERFLOW_VIDEO_SEQUENCE", "1")
    scene = Scene()
    got = render(scene, count)
    assert scene.video_sequence is not None and scene.video_sequence.frames == count
    for k in range(count):
        assert np.array_equal(want[k], got[k]), f"frame {k} differs"
    assert len({frame.tobytes() for frame in got}) >= scene.video._read
    for one in (loop, scene):
        assert one.video.format == "planar" and one.video.header == layout
        assert 18 <= one.video._read == loop.video._read <= 21
        shown = one.video.texture.get_box().texture.read()             # rows bottom-up: the last source frame read
        assert np.array_equal(np.flipud(shown), R.to_rgb(frames[one.video._read - 1], CW, CH, layout))


def test_update_shows_source_frame_k_after_k_updates(tmp_path):
    """The frame loop's path, frame by frame: the texture after update k is the restatement of source frame k (uint16 frames= here)"""
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    layout = layout_of(subsampling="420", depth=12, matrix="bt2020", chroma="linear")
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 4096, (4, R.frame_bytes(layout, CW, CH)//2)).astype(np.uint16)
    scene = bare_scene()
    video = ShaderVideo(scene=scene, frames=iter(frames), width=CW, height=CH, fps=30.0, format="yuv420p12le", yuv_matrix="bt2020", chroma="linear")
    assert video.format == "planar" and video.header == layout
    for k in range(4):
        scene.time = (k + 0.5)/30.0
        video.update()
        assert video._read == k + 1
        assert np.array_equal(np.flipud(video.texture.get_box().texture.read()), R.to_rgb(frames[k], CW, CH, layout)), k
    video.destroy()


# ---- 3. the project reads its own export ---------------------------------------------------------------------------------------------------

def test_the_project_reads_its_own_bt709_export(monkeypatch, tmp_path):
    from shaderflow_amd.exporting import ExportingHelper
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    y, x = np.mgrid[0:CH, 0:CW]
    picture = np.stack([x*8, y*14, 255 - x*8], axis=-1).astype(np.uint8)   # saturated colours, smooth: the matrix matters, the subsampling little
    clip = np.stack([np.roll(picture, 2*k, axis=1) for k in range(4)])
    Source = video_scene(lambda: dict(frames=clip, fps=FPS))
    frames = 4
    rendered = np.frombuffer(Source().main(width=W, height=H, fps=FPS, time=frames/FPS, output=bytes, top_down=True), np.uint8).reshape(frames, H, W, 3)
    made = ExportingHelper.__init__
    monkeypatch.setattr(ExportingHelper, "__init__", lambda self, *args, **kwargs: made(self, *args, **{**kwargs, "yuv_matrix": "bt709"}))
    Source().main(width=W, height=H, fps=FPS, time=frames/FPS, output=str(tmp_path/"own.yuv"), pixel_format="yuv420p", top_down=True)
    monkeypatch.setattr(ExportingHelper, "__init__", made)
    exported = np.fromfile(tmp_path/"own.yuv", np.uint8).reshape(frames, W*H*3//2)
    layout = layout_of(matrix="bt709")
    errors = {}
    for matrix in ("bt709", "bt601"):
        scene = bare_scene()
        video = ShaderVideo(scene=scene, path=tmp_path/"own.yuv", width=W, height=H, fps=FPS, yuv_matrix=matrix)
        assert video.format == ("planar" if matrix == "bt709" else "i420")
        total = 0.0
        for k in range(frames):
            scene.time = (k + 0.5)/FPS
            video.update()
            shown = np.flipud(video.texture.get_box().texture.read())
            if matrix == "bt709":
                assert np.array_equal(shown, R.to_rgb(exported[k], W, H, layout)), k
            total += float(np.abs(shown.astype(np.int64) - rendered[k].astype(np.int64)).mean())
        errors[matrix] = total/frames
        video.destroy()
    assert errors["bt709"] < errors["bt601"], errors


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------

def test_the_entry_point_refuses_by_return_code():
    from shaderflow_amd import _native as N
    lib, context = N.lib(), N.default_context()
    texture, handle = N.Handle(), N.Handle()
    N.check(lib.sfx_texture_create(context.handle, 9, 7, 3, N.U8, C.byref(texture)))
    boxes = (N.Handle*1)(texture)
    try:
        def create(w, h, **fields):
            native = N.PlanarLayout(**{"subsampling": 0, "depth": 8, "matrix": 0, "range": 0, "filter": 0, "siting": 0, **fields})
            return lib.sfx_video_create_planar(context.handle, boxes, 1, w, h, C.byref(native), 1, C.byref(handle))
        assert create(9, 7, subsampling=1) != N.OK and b"9 x 7" in lib.sfx_last_error()                  # an odd width with 4:2:2
        assert create(9, 7, subsampling=2) == N.OK                                                        # … 4:4:4 takes it
        lib.sfx_video_destroy(handle)
        assert create(9, 7, subsampling=3) == N.OK
        lib.sfx_video_destroy(handle)
        assert create(8, 7, subsampling=0) != N.OK and b"8 x 7" in lib.sfx_last_error()                  # an odd height with 4:2:0
        for field, value in (("subsampling", 4), ("subsampling", -1), ("depth", 9), ("depth", 16), ("matrix", 3), ("range", 2), ("filter", 2), ("siting", -1)):
            assert create(8, 6, **{field: value}) != N.OK and field.encode() in lib.sfx_last_error(), field
        assert create(9, 7, subsampling=3, depth=10) != N.OK and b"depth" in lib.sfx_last_error()        # deep grey
        assert lib.sfx_video_create_planar(context.handle, boxes, 1, 9, 7, None, 1, C.byref(handle)) != N.OK
        assert lib.sfx_video_create(context.handle, boxes, 1, 9, 7, N.VIDEO_PLANAR, 1, C.byref(handle)) != N.OK   # format 4 is not sfx_video_create's
        assert N.VIDEO_PLANAR == 4
    finally:
        lib.sfx_texture_destroy(texture)


def test_a_frame_of_the_wrong_size_names_the_layout():
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    scene = bare_scene()
    frames = [np.zeros(CW*CH*2 - 1, np.uint8)]
    video = ShaderVideo(scene=scene, frames=iter(frames), width=CW, height=CH, fps=30.0, format="yuv422p", yuv_matrix="bt709")
    scene.time = 1.0
    with pytest.raises(ValueError) as raised:
        video.update()
    words = str(raised.value)
    assert all(part in words for part in ("source frame 0", "yuv422p", "bt709", f"{CW} x {CH}", str(CW*CH*2), str(CW*CH*2 - 1))), words
    video.destroy()


def test_python_refusals(tmp_path):
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.video import ShaderVideo
    (tmp_path/"dv.y4m").write_bytes(b"YUV4MPEG2 W32 H18 F25:1 C420paldv\nFRAME\n" + bytes(32*18*3//2))
    with pytest.raises(ValueError, match="C420paldv"):
        ShaderVideo(scene=bare_scene(), path=tmp_path/"dv.y4m", chroma="linear")
    assert ShaderVideo(scene=bare_scene(), path=tmp_path/"dv.y4m").format == "i420"
    with pytest.raises(ValueError, match="31 x 18"):
        ShaderVideo(scene=bare_scene(), frames=iter([]), width=31, height=18, fps=30.0, format="yuv422p")
    with pytest.raises(ValueError, match="yuv411p"):
        ShaderVideo(scene=bare_scene(), frames=iter([]), width=32, height=18, fps=30.0, format="yuv411p")
    with pytest.raises(ValueError, match="bt470"):
        ShaderVideo(scene=bare_scene(), frames=iter([]), width=32, height=18, fps=30.0, format="yuv444p", yuv_matrix="bt470")
