"""
The case table of tests/test_gpu_layered.py, checked on the oracle alone (no GPU): each case is there because it reaches something a
same-size clamp layer does not — taps between texels, a wrap that differs from the clamp, a tile above a launch threshold. If one of
these stops holding, the GPU test would go on passing while holding less.
"""
import numpy as np

from oracle import binding as O
from tests import layered_cases as L


def motionblur_frames(w, h, lw, lh, temporal, seed):
    rng = np.random.default_rng(seed)
    layers = [L.noise(rng, lw, lh) for _ in range(temporal)]
    return [L.motionblur_oracle(w, h, layers, [("linear", *wrap)]*temporal) for wrap in (L.CLAMP, L.REPEAT)]


def test_motionblur_at_the_targets_size_cannot_tell_clamp_from_repeat():
    """Layers of the target's size: every tap on a texel centre, the weights 1, 0, 0, 0 — the neighbours' values never reach the frame"""
    clamp, repeat = motionblur_frames(96, 54, 96, 54, 3, seed=3)
    assert np.array_equal(clamp, repeat)
    assert clamp[..., :3].std() > 0


def test_motionblur_at_half_size_tells_clamp_from_repeat():
    clamp, repeat = motionblur_frames(96, 54, 48, 27, 3, seed=3)
    differ = np.any(clamp != repeat, axis=-1)
    assert differ.any()
    assert not differ[1:-1, 1:-1].any()                              # the border pixels only: there a neighbour is across the edge


def test_multipass_wrap_shows_on_the_blurred_half_only():
    w, h = 100, 37
    layer, background = L.noise(1, w, h), L.noise(2, 16, 9, 3)
    clamp = L.multipass_oracle(w, h, layer, background, L.CLAMP)
    repeat = L.multipass_oracle(w, h, layer, background, L.REPEAT)
    differ = np.any(clamp != repeat, axis=-1)
    assert differ[0, w//2:].any() and differ[-1, w//2:].any()         # the blur reaches over the bottom and the top edge
    assert not differ[:, :w//2].any()                                 # 1 - red of the texel under the pixel
    mixed = L.multipass_oracle(w, h, layer, background, L.MIXED)      # repeat in x only: neither of the two
    assert not np.array_equal(mixed, clamp) and not np.array_equal(mixed, repeat)
    # the left half is the property the GPU test asserts too
    assert np.array_equal(clamp[:, :w//2, 0], 255 - layer[:, :w//2, 0]) and np.array_equal(clamp[:, :w//2, 1:3], layer[:, :w//2, 1:3])


def test_multipass_layer_scale_matters():
    """130x50 over 65x25 against the same picture brought to 130x50 by a nearest copy first: other taps, other weights"""
    w, h, lw, lh = 130, 50, 65, 25
    layer, background = L.noise(4, lw, lh), L.noise(2, 16, 9, 3)
    copy = O.render("video", O.default_uniforms(w, h), {0: O.make_texture(layer, "nearest", False, False)}, w, h, threads=8)
    assert np.array_equal(copy[::2, ::2, :3], layer[..., :3]) and np.array_equal(copy[1::2, 1::2, :3], layer[..., :3])    # (alpha is 1)
    half = L.multipass_oracle(w, h, layer, background)
    full = L.multipass_oracle(w, h, copy, background)
    assert not np.array_equal(half[:, :w//2], full[:, :w//2])        # taps between texels on the left half …
    assert not np.array_equal(half[:, w//2:], full[:, w//2:])        # … and in the blur


def test_multipass_tiles_sit_on_both_sides_of_the_launch_thresholds():
    """The tile figures of the case table, by launch_multipass_layer1's formula: dynamic LDS above 48 KiB needs the function
    attribute, above 96 KiB the launch steps aside"""
    assert L.multipass_tile(128, 72, 128, 72) == (71, 15, 71*15*16)
    assert L.multipass_tile(130, 50, 65, 25)[:2] == (39, 11)
    assert L.multipass_tile(128, 72, 192, 108)[:2] == (103, 19)
    assert L.multipass_tile(128, 72, 256, 144) == (136, 23, 50048) and 48*1024 < 50048 <= 96*1024
    assert L.multipass_tile(128, 72, 384, 216) == (200, 31, 99200) and 99200 > 96*1024
    assert L.multipass_tile(100, 37, 100, 37)[2] <= 48*1024


def test_fuzz_shapes_stay_under_the_tile_cap():
    """Every seed of the GPU fuzz must take the fast kernel: ratios up to 2 keep the tile below 96 KiB, and the draw covers what it is for"""
    shapes = [L.fuzz_shape(np.random.default_rng(1000 + seed)) for seed in range(24)]
    assert all(L.multipass_tile(w, h, lw, lh)[2] <= 96*1024 for w, h, lw, lh, *_ in shapes)
    assert any(w % 64 and w > 64 for w, *_ in shapes) and any(h % 8 for _, h, *_ in shapes)
    assert {wrap for *_, wrap, _, _ in shapes} == {(False, False), (True, True), (True, False), (False, True)}
    assert {(c, np.dtype(d)) for *_, c, d in shapes} == {(c, np.dtype(d)) for c, d in L.TARGETS}
