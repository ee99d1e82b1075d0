"""
k_multipass_layer1 and k_motionblur_layer1 (csrc/layered_fast.hpp) against the oracle at the shapes where such kernels go wrong: a
block that holds both halves of the picture, partial blocks in either axis, a thread whose second row is outside, targets smaller than
a wave, layers at other sizes than the target (taps between texels, other tile sizes, the dynamic-LDS attribute, the tile cap), repeat
and mixed wrap, every render-target type, and seeded fuzz over all of it.

The kernels promise the generic chain's bits, so the bound is np.array_equal (float targets on their bit patterns), and every case
asserts which kernel ran: the fast one where it must, k_render<PlainShader<…>> where the launch has to step aside — with the same
bits. tests/test_host_layered.py checks on the oracle alone that these cases reach what they are here for.
"""
import numpy as np
import pytest

from tests import layered_cases as L
from tests.helpers import Gpu

pytestmark = pytest.mark.gpu

MULTIPASS, MOTIONBLUR = "k_multipass_layer1", "k_motionblur_layer1"


@pytest.fixture()
def gpu():
    g = Gpu()
    yield g
    g.close()


def kernel(gpu) -> str:
    return gpu.lib.sfx_last_kernel().decode()


def assert_kernel(gpu, fast: str | None):
    name = kernel(gpu)
    if fast:
        assert name == fast, name
    else:
        assert "k_render<" in name and "Plain" in name, name


def report(got, want) -> str:
    differ = np.any(L.bits(got) != L.bits(want), axis=-1)
    rows, columns = np.nonzero(differ)
    where = f"columns {columns.min()}..{columns.max()}, rows {rows.min()}..{rows.max()}" if differ.any() else "nowhere"
    return f"{int(differ.sum())}/{differ.size} pixels differ ({where})"


def assert_same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(L.bits(got), L.bits(want)), report(got, want)


# ---- multipass.frag, layer 1 -------------------------------------------------------------------------------------------------------------

def multipass_gpu(gpu, w, h, layer, background, wrap=L.CLAMP, filter="linear", components=4, dtype=np.uint8):
    prog, fallback = gpu.program("multipass")
    assert not fallback
    gpu.set_uniforms(prog, L.multipass_uniforms(w, h))
    assert gpu.bind(prog, "background", gpu.texture(background))
    assert gpu.bind(prog, "iScreen0x0", gpu.texture(layer, filter, *wrap))
    return gpu.render(prog, w, h, comps=components, dtype=dtype, layer=1)


def check_multipass(gpu, w, h, lw, lh, wrap, seed, fast=MULTIPASS, components=4, dtype=np.uint8, filter="linear", layer=None):
    rng = np.random.default_rng(seed)
    if layer is None:
        layer = L.noise(rng, lw, lh)
    background = L.noise(rng, 16, 9, 3)
    want = L.multipass_oracle(w, h, layer, background, wrap, filter, components, dtype)
    got = multipass_gpu(gpu, w, h, layer, background, wrap, filter, components, dtype)
    assert_kernel(gpu, fast)
    assert_same_bits(got, want)
    assert want.size < 64 or L.bits(want)[..., :3].std() > 0            # (a picture, not a constant)
    return got, layer


# (target, layer or None for the target's size): see the module's docstring and, for the tile figures, test_host_layered.py
MULTIPASS_SHAPES = [
    ((64, 8), None),            # exactly one block; left and right pixels share it
    ((100, 37), None),          # the centre column inside block column 0; 36 columns in block column 1; 5 rows in the last block row
    ((101, 37), None),          # odd width: gluv.x == 0 at column 50 goes right
    ((65, 9), None),            # one pixel column and one pixel row of overhang
    ((257, 33), None),          # five block columns, overhang of 1 in both axes
    ((1, 1), None), ((2, 3), None),     # smaller than a wave
    ((130, 50), (65, 25)),      # half-size layer: taps between texels, tile 39 x 11
    ((128, 72), (192, 108)),    # 1.5 x: tile 103 x 19
    ((128, 72), (256, 144)),    # 2 x: tile 136 x 23 = 50 048 bytes, the dynamic-LDS attribute
    ((300, 17), (3, 2)),        # tiny layer: the window starts two texels below zero, repeat wraps by a whole period of the 2 rows
    ((100, 37), (80, 45)),      # non-integer ratio, another aspect
]


def shape_id(shape) -> str:
    (w, h), layer = shape
    return f"{w}x{h}" + (f"-from-{layer[0]}x{layer[1]}" if layer else "")


@pytest.mark.parametrize("wrap", L.WRAPS, ids=L.wrap_id)
@pytest.mark.parametrize("shape", MULTIPASS_SHAPES, ids=shape_id)
def test_multipass_layer1_shapes_bit_exact(gpu, shape, wrap):
    (w, h), (lw, lh) = shape[0], shape[1] or shape[0]
    got, layer = check_multipass(gpu, w, h, lw, lh, wrap, seed=w*1000 + h)
    if (w, h, lw, lh) == (100, 37, 100, 37) and wrap == L.CLAMP:
        # multipass.frag:38-39 in a block that also blurs: 1 - red, green and blue untouched
        assert np.array_equal(got[:, :w//2, 0], 255 - layer[:, :w//2, 0]) and np.array_equal(got[:, :w//2, 1:3], layer[:, :w//2, 1:3])
        assert not np.array_equal(got[:, w//2:, :3], layer[:, w//2:, :3])


@pytest.mark.parametrize("wrap", L.WRAPS, ids=L.wrap_id)
def test_multipass_tile_above_the_cap_steps_aside_with_the_same_bits(gpu, wrap):
    """3 x: a tile of 200 x 31 texels = 99 200 bytes, above the 96 KiB the launch allows itself"""
    assert L.multipass_tile(128, 72, 384, 216)[2] > 96*1024
    check_multipass(gpu, 128, 72, 384, 216, wrap, seed=5, fast=None)


@pytest.mark.parametrize("components,dtype", L.TARGETS[1:], ids=["rgb8", "rgba16f", "rgba32f"])
def test_multipass_layer1_target_types_bit_exact(gpu, components, dtype):
    check_multipass(gpu, 100, 37, 100, 37, L.MIXED, seed=6, components=components, dtype=dtype)


@pytest.mark.parametrize("what", ["nearest", "rgb8", "rgba32f"])
def test_multipass_other_layers_step_aside_with_the_same_bits(gpu, what):
    w, h = 100, 37
    layer = {"nearest": L.noise(7, w, h), "rgb8": L.noise(7, w, h, 3), "rgba32f": L.noise(7, w, h, 4, np.float32)}[what]
    check_multipass(gpu, w, h, w, h, L.CLAMP, seed=8, fast=None, filter="nearest" if what == "nearest" else "linear", layer=layer)


@pytest.mark.parametrize("seed", range(24))
def test_multipass_layer1_fuzz_bit_exact(gpu, seed):
    rng = np.random.default_rng(1000 + seed)
    w, h, lw, lh, wrap, components, dtype = L.fuzz_shape(rng)
    check_multipass(gpu, w, h, lw, lh, wrap, seed=rng, components=components, dtype=dtype)


# ---- motionblur.frag, layer 1 ------------------------------------------------------------------------------------------------------------

def motionblur_gpu(gpu, w, h, layers, samplers, components=4, dtype=np.uint8):
    temporal = len(layers)
    prog, fallback = gpu.program("motionblur")
    assert not fallback
    gpu.set_uniforms(prog, L.motionblur_uniforms(w, h, temporal))
    assert gpu.set_values(prog, "iScreenTemporal", temporal, integer=True)
    for t in range(temporal):
        assert gpu.bind(prog, f"iScreen{t}x0", gpu.texture(layers[t], *samplers[t]))
    return gpu.render(prog, w, h, comps=components, dtype=dtype, layer=1)


def check_motionblur(gpu, w, h, layers, samplers, fast=MOTIONBLUR, components=4, dtype=np.uint8):
    want = L.motionblur_oracle(w, h, layers, samplers, components, dtype)
    got = motionblur_gpu(gpu, w, h, layers, samplers, components, dtype)
    assert_kernel(gpu, fast)
    assert_same_bits(got, want)
    assert want.size < 64 or L.bits(want)[..., :3].std() > 0            # (a picture, not a constant)
    return want


def history(seed, lw, lh, temporal):
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    return [L.noise(rng, lw, lh) for _ in range(temporal)]


@pytest.mark.parametrize("w,h,lw,lh,temporal,wrap", [
    (64, 4, 64, 4, 2, L.CLAMP),             # exactly one block
    (65, 5, 65, 5, 3, L.CLAMP),             # overhang of 1 in both axes; an odd count under `#pragma unroll 2`
    (1, 1, 1, 1, 1, L.CLAMP),               # smallest
    (96, 54, 192, 108, 11, L.CLAMP),        # 2 x layers, odd count
    (96, 54, 80, 45, 12, L.CLAMP),          # non-integer ratio, full depth
    (96, 54, 80, 45, 12, L.MIXED),
    (130, 7, 2, 2, 12, L.REPEAT),           # tiny layers
], ids=lambda v: L.wrap_id(v) if isinstance(v, tuple) else str(v))
def test_motionblur_layer1_shapes_bit_exact(gpu, w, h, lw, lh, temporal, wrap):
    check_motionblur(gpu, w, h, history(w*100 + temporal, lw, lh, temporal), [("linear", *wrap)]*temporal)


def test_motionblur_half_size_layers_every_wrap_bit_exact(gpu):
    """96x54 over 48x27: every tap between texels (both weights of an axis non-zero), and the border pixels' neighbours across the edge,
    where clamp and repeat part — asserted, so that the case cannot decay into one that does not look at the wrap"""
    w, h, temporal = 96, 54, 3
    layers = history(21, 48, 27, temporal)
    frames = {wrap: check_motionblur(gpu, w, h, layers, [("linear", *wrap)]*temporal) for wrap in L.WRAPS}
    assert not np.array_equal(frames[L.CLAMP], frames[L.REPEAT])
    assert not np.array_equal(frames[L.MIXED], frames[L.CLAMP]) and not np.array_equal(frames[L.MIXED], frames[L.REPEAT])


@pytest.mark.parametrize("components,dtype", L.TARGETS[1:], ids=["rgb8", "rgba16f", "rgba32f"])
def test_motionblur_layer1_target_types_bit_exact(gpu, components, dtype):
    check_motionblur(gpu, 96, 54, history(22, 48, 27, 3), [("linear", True, False)]*3, components=components, dtype=dtype)


@pytest.mark.parametrize("what", ["size", "wrap", "nearest"])
def test_motionblur_unlike_layers_step_aside_with_the_same_bits(gpu, what):
    """The fast kernel addresses all layers at once: one layer of another size or sampler state sends the launch to the generic kernel"""
    w, h = 96, 54
    rng = np.random.default_rng(23)
    sizes = [(48, 27), (48, 27), (96, 54)] if what == "size" else [(48, 27)]*3
    layers = [L.noise(rng, lw, lh) for lw, lh in sizes]
    samplers = [("linear", False, False)]*3
    if what == "wrap":
        samplers[1] = ("linear", True, False)
    if what == "nearest":
        samplers[2] = ("nearest", False, False)
    check_motionblur(gpu, w, h, layers, samplers, fast=None)


@pytest.mark.parametrize("seed", range(16))
def test_motionblur_layer1_fuzz_bit_exact(gpu, seed):
    rng = np.random.default_rng(2000 + seed)
    w, h, lw, lh, wrap, components, dtype = L.fuzz_shape(rng)
    temporal = int(rng.integers(1, 13))
    check_motionblur(gpu, w, h, history(rng, lw, lh, temporal), [("linear", *wrap)]*temporal, components=components, dtype=dtype)
