"""
Planar sources on the host (shaderflow_amd/planarsource.py) and the definition's restatement (tests/planar_ref.py):

  1. the Y4M parser: every tag it reads and every tag it refuses (naming it), `frame_bytes` per layout, the reader on a two-frame file
     of each layout with a truncated third frame;
  2. the restatement at the I420 layout is the `(298 C + 409 E + 128) >> 8` formulas, restated here, bit for bit;
  3. the coefficient tables the definition lists, and every layout's intermediates below 2^31;
  4. the float64 witness: where the real-valued conversion lies in [0, 255] the integer rule is within
     1/2 + sum of max|operand| 2^-(S+1) of it — a bound computed from the layout (at most 1.5 levels at 8 bit, 0.75 deeper);
  5. the filter: linear on constant chroma and on 4:4:4 is nearest; a horizontal chroma ramp gives the quarter-weight values written
     out by hand for both sitings, edges included.
"""
from __future__ import annotations

import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import planar_ref as R                                                 # noqa: E402

from shaderflow_amd.planarsource import FORMAT_NAMES, PlanarClip, PlanarLayout, parse_y4m   # noqa: E402

W, H = 6, 4
CORNERS = list(itertools.product((0.0, 1.0), repeat=3))                # luma, cb, cr at either end of the sample range


def random_frame(rng, layout, w, h):
    top = 2**layout.depth - 1
    count = R.frame_bytes(layout, w, h)//layout.sample_bytes
    return rng.integers(0, top + 1, count).astype(np.uint16 if layout.depth > 8 else np.uint8)


def constant_frame(layout, w, h, luma, cb, cr):
    cw, ch = R.chroma_extents(layout, w, h)
    dtype = np.uint16 if layout.depth > 8 else np.uint8
    return np.concatenate([np.full(w*h, luma, dtype), np.full(cw*ch, cb, dtype), np.full(cw*ch, cr, dtype)])


# ---- 1. the parser and the reader ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag, subsampling, depth, siting, nearest_only", [
    (None, "420", 8, "centre", False), ("C420", "420", 8, "centre", False), ("C420jpeg", "420", 8, "centre", False),
    ("C420mpeg2", "420", 8, "left", False), ("C420paldv", "420", 8, "centre", True), ("C422", "422", 8, "left", False),
    ("C444", "444", 8, "centre", False), ("Cmono", "mono", 8, "centre", False),
    ("C420p10", "420", 10, "centre", False), ("C422p10", "422", 10, "left", False), ("C444p10", "444", 10, "centre", False),
    ("C420p12", "420", 12, "centre", False), ("C422p12", "422", 12, "left", False), ("C444p12", "444", 12, "centre", False),
])
def test_y4m_tags_that_are_read(tag, subsampling, depth, siting, nearest_only):
    line = f"YUV4MPEG2 W64 H36 F30000:1001 Ip A1:1{' ' + tag if tag else ''} XYSCSS=ANY\n".encode()
    width, height, fps, fields = parse_y4m(line)
    assert (width, height) == (64, 36) and fps == 30000/1001
    assert (fields["subsampling"], fields["depth"], fields["siting"]) == (subsampling, depth, siting)
    assert fields["range"] is None and (fields["nearest_only"] == tag if nearest_only else fields["nearest_only"] is None)


@pytest.mark.parametrize("tag, value", [("XCOLORRANGE=FULL", "full"), ("XCOLORRANGE=LIMITED", "limited"), ("XCOLORRANGE=full", "full")])
def test_y4m_range_tags(tag, value):
    assert parse_y4m(f"YUV4MPEG2 W64 H36 F25:1 C444 {tag}\n".encode())[3]["range"] == value


@pytest.mark.parametrize("tag", ["Ii", "It", "Ib", "Im", "C444alpha", "C411", "C420p9", "C420p14", "C420p16", "C422p16", "C444p14",
                                 "Cmono9", "Cmono10", "Cmono12", "Cmono16"])
def test_y4m_tags_that_are_refused_are_named(tag):
    with pytest.raises(ValueError, match=tag):
        parse_y4m(f"YUV4MPEG2 W64 H36 F25:1 {tag}\n".encode())


@pytest.mark.parametrize("header, names", [(b"YUV4MPEG2 W63 H36 F25:1 C422\n", "W63"), (b"YUV4MPEG2 W64 H35 F25:1 C420p10\n", "H35"),
                                           (b"YUV4MPEG2 W63 H36 F25:1\n", "W63")])
def test_y4m_odd_extents_on_a_subsampled_axis_are_refused(header, names):
    with pytest.raises(ValueError, match=names):
        parse_y4m(header)
    assert parse_y4m(b"YUV4MPEG2 W63 H35 F25:1 C444\n")[:2] == (63, 35) and parse_y4m(b"YUV4MPEG2 W64 H35 F25:1 C422\n")[:2] == (64, 35)
    assert parse_y4m(b"YUV4MPEG2 W1 H1 F25:1 Cmono\n")[:2] == (1, 1)


@pytest.mark.parametrize("name, subsampling, depth, expected", [
    ("yuv420p", "420", 8, 64*36*3//2), ("yuv422p", "422", 8, 64*36*2), ("yuv444p", "444", 8, 64*36*3), ("gray", "mono", 8, 64*36),
    ("yuv420p10le", "420", 10, 64*36*3), ("yuv422p10le", "422", 10, 64*36*4), ("yuv444p10le", "444", 10, 64*36*6),
    ("yuv420p12le", "420", 12, 64*36*3), ("yuv422p12le", "422", 12, 64*36*4), ("yuv444p12le", "444", 12, 64*36*6),
])
def test_frame_bytes_per_layout(name, subsampling, depth, expected):
    layout = PlanarLayout.from_format(name)
    assert name in FORMAT_NAMES and (layout.subsampling, layout.depth) == (subsampling, depth)
    assert layout.frame_bytes(64, 36) == expected == R.frame_bytes(layout, 64, 36)
    assert layout.is_i420 == (name == "yuv420p")


def test_layouts_refuse_what_they_do_not_name():
    for name in ("yuv411p", "gray10le", "yuv420p16le", "rgb24", "yuv420p10"):
        with pytest.raises(ValueError, match=name):
            PlanarLayout.from_format(name)
    for field, value in (("matrix", "bt470"), ("range", "tv"), ("chroma", "cubic"), ("siting", "top"), ("depth", 9)):
        with pytest.raises(ValueError, match=str(value)):
            PlanarLayout(**{field: value})
    assert not PlanarLayout(matrix="bt709").is_i420 and not PlanarLayout(chroma="linear").is_i420 and not PlanarLayout(range="full").is_i420
    assert PlanarLayout(siting="left").is_i420                         # (nothing reads the siting without the filter)
    with pytest.raises(ValueError, match="63 x 36"):
        PlanarLayout(subsampling="422").check_extents(63, 36)
    with pytest.raises(ValueError, match="64 x 35"):
        PlanarLayout().check_extents(64, 35)
    PlanarLayout(subsampling="422").check_extents(64, 35)
    PlanarLayout(subsampling="444").check_extents(1, 1)


@pytest.mark.parametrize("tag, name", [("C420jpeg", "yuv420p"), ("C422", "yuv422p"), ("C444", "yuv444p"), ("Cmono", "gray"),
                                       ("C420p10", "yuv420p10le"), ("C422p10", "yuv422p10le"), ("C444p12", "yuv444p12le")])
def test_the_reader_on_two_frames_and_a_truncated_third(tmp_path, tag, name):
    layout = PlanarLayout.from_format(name)
    rng = np.random.default_rng(len(tag))
    frames = [random_frame(rng, layout, 16, 6) for _ in range(3)]
    size = layout.frame_bytes(16, 6)
    raw = [frame.astype("<u2" if layout.depth > 8 else np.uint8).tobytes() for frame in frames]
    assert all(len(one) == size for one in raw)
    with open(tmp_path/"clip.y4m", "wb") as file:
        file.write(f"YUV4MPEG2 W16 H6 F24:1 Ip {tag} XCOLORRANGE=FULL\n".encode())
        file.write(b"FRAME\n" + raw[0] + b"FRAME Xcomment\n" + raw[1] + b"FRAME\n" + raw[2][:size//2])
    (tmp_path/"clip.yuv").write_bytes(raw[0] + raw[1] + raw[2][:size - 1])
    for clip in (PlanarClip(tmp_path/"clip.y4m", matrix="bt709", chroma="linear"),
                 PlanarClip(tmp_path/"clip.yuv", 16, 6, 24.0, format=name, matrix="bt709", range="full", chroma="linear")):
        assert (clip.width, clip.height, clip.fps, clip.frame_bytes) == (16, 6, 24.0, size)
        assert (clip.layout.subsampling, clip.layout.depth, clip.layout.matrix, clip.layout.range, clip.layout.chroma) == \
               (layout.subsampling, layout.depth, "bt709", "full", "linear")
        got = list(clip)
        assert len(got) == 2 and all(one.dtype == np.uint8 and one.tobytes() == want for one, want in zip(got, raw))
        assert clip.readinto(np.empty(size, np.uint8)) is False


def test_the_reader_takes_the_files_range_unless_told(tmp_path):
    frame = bytes(16*6*3)
    (tmp_path/"full.y4m").write_bytes(b"YUV4MPEG2 W16 H6 F24:1 C444 XCOLORRANGE=FULL\nFRAME\n" + frame)
    (tmp_path/"none.y4m").write_bytes(b"YUV4MPEG2 W16 H6 F24:1 C444\nFRAME\n" + frame)
    assert PlanarClip(tmp_path/"full.y4m").layout.range == "full" and PlanarClip(tmp_path/"none.y4m").layout.range == "limited"
    assert PlanarClip(tmp_path/"full.y4m", range="limited").layout.range == "limited"
    assert PlanarClip(tmp_path/"none.y4m", range="full").layout.range == "full"


def test_paldv_is_nearest_only(tmp_path):
    (tmp_path/"dv.y4m").write_bytes(b"YUV4MPEG2 W16 H6 F25:1 C420paldv\nFRAME\n" + bytes(16*6*3//2))
    assert PlanarClip(tmp_path/"dv.y4m").layout.is_i420
    with pytest.raises(ValueError, match="C420paldv"):
        PlanarClip(tmp_path/"dv.y4m", chroma="linear")


def test_raw_files_need_their_geometry_and_even_extents(tmp_path):
    (tmp_path/"clip.yuv").write_bytes(bytes(1000))
    with pytest.raises(ValueError, match="width"):
        PlanarClip(tmp_path/"clip.yuv", format="yuv444p")
    with pytest.raises(ValueError, match="15 x 6"):
        PlanarClip(tmp_path/"clip.yuv", 15, 6, 24.0, format="yuv422p")


# ---- 2. the special case ---------------------------------------------------------------------------------------------------------------

def i420_formulas(frame, w, h):
    """Today's I420 conversion, restated: C = Y - 16, D = U - 128, E = V - 128, (298 C + 409 E + 128) >> 8 and its two siblings"""
    frame = np.asarray(frame, np.uint8).astype(np.int64)
    q = (w//2)*(h//2)
    y = frame[:w*h].reshape(h, w)
    u = frame[w*h:w*h + q].reshape(h//2, w//2).repeat(2, axis=0).repeat(2, axis=1)
    v = frame[w*h + q:].reshape(h//2, w//2).repeat(2, axis=0).repeat(2, axis=1)
    c, d, e = y - 16, u - 128, v - 128
    return np.clip(np.stack([(298*c + 409*e + 128) >> 8, (298*c - 100*d - 208*e + 128) >> 8, (298*c + 516*d + 128) >> 8], axis=-1), 0, 255).astype(np.uint8)


def test_the_i420_layout_is_todays_formulas_bit_for_bit():
    layout, rng = PlanarLayout(), np.random.default_rng(1)
    assert layout.is_i420
    w, h = 34, 6
    frames = [random_frame(rng, layout, w, h) for _ in range(4)]
    frames += [constant_frame(layout, w, h, 255*a, 255*b, 255*c).astype(np.uint8) for a, b, c in CORNERS]
    for chroma in ((255, 0), (0, 255)):                                # random luma over extreme chroma: both clips
        mixed = random_frame(rng, layout, w, h)
        mixed[w*h:w*h + (w//2)*(h//2)], mixed[w*h + (w//2)*(h//2):] = chroma
        frames.append(mixed)
    for frame in frames:
        assert np.array_equal(R.to_rgb(frame, w, h, layout), i420_formulas(frame, w, h))
    values = np.arange(-200000, 200001, dtype=np.int64)                # the identity behind it
    assert np.array_equal((16*values + 2048) >> 12, (values + 128) >> 8)


# ---- 3. the coefficients ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fields, table", [
    (dict(), (298, 409, 100, 208, 516)),
    (dict(matrix="bt709"), (298, 459, 55, 136, 541)),
    (dict(range="full"), (256, 359, 88, 183, 454)),
    (dict(depth=10), (4769, 6537, 1605, 3330, 8263)),
])
def test_the_coefficient_tables(fields, table):
    q = R.coefficients(PlanarLayout(**fields))
    assert (q["cy"], q["crv"], q["cgu"], q["cgv"], q["cbu"]) == table


ALL_LAYOUTS = [PlanarLayout(depth=depth, matrix=matrix, range=range_) for depth in (8, 10, 12) for matrix in ("bt601", "bt709", "bt2020")
               for range_ in ("limited", "full")]


@pytest.mark.parametrize("layout", ALL_LAYOUTS, ids=lambda one: one.describe().replace(" ", "-"))
def test_every_layouts_intermediates_fit_32_bits(layout):
    q = R.coefficients(layout)
    assert (q["offset"], q["mid"], q["S"]) == (0 if layout.range == "full" else 16 << (layout.depth - 8), 1 << (layout.depth - 1), {8: 8, 10: 14, 12: 16}[layout.depth])
    assert R.intermediates_peak(layout) < 2**31


# ---- 4. the float64 witness ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ALL_LAYOUTS, ids=lambda one: one.describe().replace(" ", "-"))
@pytest.mark.parametrize("subsampling, chroma", [("420", "linear"), ("444", "nearest")])
def test_the_integer_rule_against_the_real_valued_conversion(layout, subsampling, chroma):
    from attrs import evolve
    layout = evolve(layout, subsampling=subsampling, chroma=chroma)
    rng, top = np.random.default_rng(layout.depth), 2**layout.depth - 1
    bound = R.error_bound(layout)
    assert bound.max() <= (1.5 if layout.depth == 8 else 0.75)
    frames = [random_frame(rng, layout, 18, 8) for _ in range(6)]
    frames += [constant_frame(layout, 18, 8, int(top*a), int(top*b), int(top*c)) for a, b, c in CORNERS]
    q = R.coefficients(layout)                                         # … and frames near the grey axis, where all three channels are in range
    frames += [constant_frame(layout, 18, 8, luma, q["mid"] + k, q["mid"] - k) for luma in (q["offset"], top//2, top - q["offset"]) for k in (0, 3)]
    inside = 0
    for frame in frames:
        exact, got = R.to_rgb_exact(frame, 18, 8, layout), R.to_rgb(frame, 18, 8, layout).astype(np.float64)
        valid = (exact >= 0.0) & (exact <= 255.0)
        inside += int(valid.sum())
        assert (np.abs(got - exact)[valid] <= np.broadcast_to(bound, exact.shape)[valid]).all()
    assert inside > 1000


def test_grey_frames_have_three_equal_channels():
    layout, rng = PlanarLayout(subsampling="mono", range="full"), np.random.default_rng(3)
    frame = random_frame(rng, layout, 17, 3)
    rgb = R.to_rgb(frame, 17, 3, layout)
    assert np.array_equal(rgb[..., 0], frame.reshape(3, 17)) and np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 1], rgb[..., 2])
    limited = PlanarLayout(subsampling="mono")
    exact = R.to_rgb_exact(frame, 17, 3, limited)
    valid = (exact >= 0) & (exact <= 255)
    assert (np.abs(R.to_rgb(frame, 17, 3, limited) - exact)[valid] <= R.error_bound(limited)[0]).all()


# ---- 5. the filter ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("subsampling", ["420", "422"])
@pytest.mark.parametrize("siting", ["centre", "left"])
def test_linear_on_constant_chroma_is_nearest(subsampling, siting):
    rng = np.random.default_rng(4)
    nearest, linear = PlanarLayout(subsampling=subsampling, matrix="bt709"), PlanarLayout(subsampling=subsampling, matrix="bt709", chroma="linear", siting=siting)
    frame = random_frame(rng, nearest, 18, 6)
    cw, ch = R.chroma_extents(nearest, 18, 6)
    frame[18*6:18*6 + cw*ch], frame[18*6 + cw*ch:] = 77, 201
    assert np.array_equal(R.to_rgb(frame, 18, 6, linear), R.to_rgb(frame, 18, 6, nearest))


def test_linear_on_444_is_nearest():
    rng = np.random.default_rng(5)
    nearest, linear = PlanarLayout(subsampling="444", depth=10), PlanarLayout(subsampling="444", depth=10, chroma="linear", siting="left")
    frame = random_frame(rng, nearest, 17, 5)
    assert np.array_equal(R.to_rgb(frame, 17, 5, linear), R.to_rgb(frame, 17, 5, nearest))


@pytest.mark.parametrize("siting, sixteenths", [
    # chroma samples 10, 50, 90 across a 6-pixel row, vertical weight 4 (4:2:2): quarters (1, 3) / (3, 1), the edges clamped
    ("centre", [4*(1*10 + 3*10), 4*(3*10 + 1*50), 4*(1*10 + 3*50), 4*(3*50 + 1*90), 4*(1*50 + 3*90), 4*(3*90 + 1*90)]),
    # quarters 4 / (2, 2), the last sample's right neighbour clamped
    ("left", [4*4*10, 4*(2*10 + 2*50), 4*4*50, 4*(2*50 + 2*90), 4*4*90, 4*(2*90 + 2*90)]),
])
def test_a_horizontal_chroma_ramp_by_hand(siting, sixteenths):
    w, h = 6, 2
    ramp = np.array([[10, 50, 90], [10, 50, 90]], np.int64)
    for subsampling in ("422", "420"):
        layout = PlanarLayout(subsampling=subsampling, chroma="linear", siting=siting)
        plane = ramp if subsampling == "422" else ramp[:1]             # (4:2:0: one chroma row, so the vertical taps both land on it)
        got = R.chroma_sixteenths(plane, w, h, layout)
        assert np.array_equal(got, np.array([sixteenths, sixteenths], np.int64)), (subsampling, got)
    # … and through the whole conversion: the blue channel of a mid-grey frame follows Cb's sixteenths
    layout = PlanarLayout(subsampling="422", chroma="linear", siting=siting, range="full")
    frame = np.concatenate([np.full(w*h, 128, np.uint8), ramp.astype(np.uint8).reshape(-1), np.full(6, 128, np.uint8)])
    q = R.coefficients(layout)
    want = np.clip([(16*q["cy"]*128 + q["cbu"]*(c - 16*128) + 2048) >> 12 for c in sixteenths], 0, 255)
    assert np.array_equal(R.to_rgb(frame, w, h, layout)[0, :, 2], want) and np.array_equal(R.to_rgb(frame, w, h, layout)[0, :, 0], np.full(w, 128))


def test_vertical_linear_is_the_centre_rule_on_420():
    layout = PlanarLayout(subsampling="420", chroma="linear", siting="left")
    plane = np.array([[20], [60], [100]], np.int64)                    # a 2 x 6 frame: three chroma rows of one sample
    got = R.chroma_sixteenths(plane, 2, 6, layout)
    rows = [4*(1*20 + 3*20), 4*(3*20 + 1*60), 4*(1*20 + 3*60), 4*(3*60 + 1*100), 4*(1*60 + 3*100), 4*(3*100 + 1*100)]
    assert np.array_equal(got[:, 0], rows)
    assert np.array_equal(got[:, 1], rows)                             # (left siting, odd x: (2, 2) on the same clamped sample)
