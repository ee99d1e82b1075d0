"""
The GLSL 3.30 §8.7 texture lookups of translated fragments ON THE DEVICE: the probes of tests/texture_cases.py compiled for gfx950
the way every fragment outside the registry is, held to (1) the x86 host build's bits, (2) the exact-arithmetic restatement and the
identities on their own, (3) bias and implicit derivatives — what the host build cannot witness — as identities on the quad kernels,
(4) the Python API with a mipmapped ShaderTexture, with and without the LDS tile, (5) examples/scenes.py::Glow against the host
build's frames.

On a texture with a chain `texture`, `textureOffset` and their Proj forms take the level of detail from the quad's differences; a
probe's neighbouring pixels hold unrelated rows of the table, so those forms on those textures are compared with nothing here (the
host build reads level 0 for them) — test 3 holds them through textureGrad and textureLod instead.
"""
import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import _native as N
from tests import texture_cases as T
from tests import texture_ref as R
from tests.helpers import Gpu
from tests.test_gpu_translated import load
from tests.test_host_texture import CACHE, PROBES, host_results

pytestmark = pytest.mark.gpu
F = np.float32


class Device:
    def __init__(self):
        self.gpu = Gpu()
        self.programs, self.textures = {}, {}

    def program(self, key: str, glsl: str, uniforms=T.PROBE_UNIFORMS):
        if key not in self.programs:
            self.programs[key], _ = load(self.gpu, glsl, uniforms)
            self.gpu.set_uniforms(self.programs[key], O.default_uniforms(T.WIDTH, T.HEIGHT))
        return self.programs[key]

    def texture(self, data: np.ndarray, filter: str, repeat_x: bool, repeat_y: bool, chain: bool = False):
        key = (data.tobytes(), data.shape, data.dtype.str, filter, repeat_x, repeat_y, chain)
        if key not in self.textures:
            handle = self.gpu.texture(data, filter, repeat_x, repeat_y)
            if chain:
                N.check(self.gpu.lib.sfx_texture_build_mipmaps(handle))
                N.check(self.gpu.lib.sfx_texture_params(handle, 2 if filter == "linear" else 3, int(repeat_x), int(repeat_y)))
            self.textures[key] = handle
        return self.textures[key]

    def run(self, probe: str, config: T.Config, form: int, operands: np.ndarray, gradients: np.ndarray, data=None) -> np.ndarray:
        prog = self.program(probe, T.probe_glsl(PROBES[probe]))
        assert self.gpu.bind(prog, "tex", self.texture(config.data if data is None else data, config.filter, config.repeat_x, config.repeat_y, config.chain))
        assert self.gpu.bind(prog, "operands", self.texture(operands, "nearest", False, False))
        assert self.gpu.bind(prog, "gradients", self.texture(gradients, "nearest", False, False))
        assert self.gpu.set_values(prog, "form", form, integer=True)
        return self.gpu.render(prog, T.WIDTH, T.HEIGHT, comps=4, dtype=F).reshape(T.ROWS, 4)

    def close(self):
        for prog in self.programs.values():
            N.check(self.gpu.lib.sfx_program_destroy(prog))
        self.gpu.close()


@pytest.fixture(scope="module")
def device():
    d = Device()
    try:
        yield d
    finally:
        d.close()


@pytest.fixture(scope="module")
def explicit(device):
    return T.evaluate(device.run, "explicit", T.EXPLICIT_FORMS)


@pytest.fixture(scope="module")
def proj(device):
    return T.evaluate(device.run, "proj", T.PROJ_FORMS)


def test_device_returns_its_operands_bit_for_bit(explicit):
    T.check_echo(explicit)


def test_device_equals_the_host_build_bit_for_bit(explicit, proj):
    for probe, results in (("explicit", explicit), ("proj", proj)):
        host = host_results(probe)
        for (config, name), got in results.items():
            if not T.implicit(config, name):
                T.assert_same_bits(got, host[config, name], (config.name, name, "device (got) against the x86 host build (want)"))


def test_device_against_the_restatement_and_the_identities_on_its_own(device, explicit, proj):
    T.check_reference(explicit, skip_implicit=True)
    T.check_projective(device.run, explicit, proj, skip_implicit=True)
    T.check_identities(device.run, explicit)


@pytest.mark.parametrize("size,filter", [((8, 8), "linear"), ((16, 4), "linear"), ((8, 8), "nearest"), ((16, 4), "nearest")])
def test_bias_and_implicit_derivatives_are_the_explicit_forms(device, size, filter):
    """texture(s, uv) = textureGrad(s, uv, dFdx(uv), dFdy(uv)) and texture(s, uv, b) = textureLod(s, uv, lambda_base + b), bit for
    bit, on power-of-two extents (scaling by them is exact) — and the probe's lambda_base really runs from magnification through
    every pair of levels to beyond the top"""
    data = T._data(size[0], size[1], "rgba8")
    prog = device.program("bias", T.BIAS_GLSL, [("sampler2D", "tex"), ("int", "form")])
    assert device.gpu.bind(prog, "tex", device.texture(data, filter, True, False, chain=True))
    frames = {}
    for form in (0, 1, 2):
        assert device.gpu.set_values(prog, "form", form, integer=True)
        frames[form] = device.gpu.render(prog, T.WIDTH, T.HEIGHT, comps=4, dtype=F)
    # the coordinates are the ones tests/test_host_texture.py checks the coverage of, and lambda_base is the restatement's
    assert np.array_equal(T.bits(frames[1][..., :2]), T.bits(T.bias_uv())), "uv: device against the numpy restatement"
    lam = T.quad_lambda(T.bias_uv(), size)
    assert np.array_equal(T.bits(lam), T.bits(frames[2][..., 0])), "lambda_base: device against the restatement"
    assert T.covers_every_level(lam, max(size).bit_length() - 1)
    for k, what in enumerate(["texture = textureGrad of the quad's differences", *[f"texture(bias {b}) = textureLod(base + {b})" for b in T.BIAS_VALUES]]):
        wrong = np.argwhere(frames[0][..., k] != 0)
        assert wrong.size == 0, (what, f"{len(wrong)} pixels differ, first (y, x) = {wrong[0]}, lambda_base there {lam[tuple(wrong[0])]}")


def test_the_tile_changes_nothing(device, monkeypatch):
    """the textureOffset blur with the LDS tile wished off and forced: the same floats, and the host build's"""
    config = next(c for c in T.CONFIGS if not c.chain and c.filter == "linear" and c.width == 8)
    frames = {}
    for wish in ("0", "tex"):
        monkeypatch.setenv("SHADERFLOW_JIT_TILE", wish)
        prog, translation = load(device.gpu, T.BLUR_GLSL, [("sampler2D", "tex")])
        assert translation.tiled_sampler == (None if wish == "0" else "tex")
        device.gpu.set_uniforms(prog, O.default_uniforms(T.WIDTH, T.HEIGHT))
        assert device.gpu.bind(prog, "tex", device.texture(config.data, config.filter, config.repeat_x, config.repeat_y))
        frames[wish] = device.gpu.render(prog, T.WIDTH, T.HEIGHT, comps=4, dtype=F)
        N.check(device.gpu.lib.sfx_program_destroy(prog))
    assert np.array_equal(T.bits(frames["0"]), T.bits(frames["tex"]))
    monkeypatch.setenv("SHADERFLOW_JIT_TILE", "0")
    host = host_fragment(T.BLUR_GLSL, [("sampler2D", "tex")])
    host.set_uniforms(O.default_uniforms(T.WIDTH, T.HEIGHT))
    assert host.bind("tex", config.data, config.filter, config.repeat_x, config.repeat_y)
    assert np.array_equal(T.bits(frames["0"]), T.bits(host.render_float(T.WIDTH, T.HEIGHT)))


def host_fragment(glsl: str, uniforms) -> "TextureHostFragment":
    from shaderflow_amd import glsl2hip as G
    from tests.texture_host import TextureHostFragment
    return TextureHostFragment(G.translate(glsl, uniforms), CACHE)


def pixel_centres(n: int) -> np.ndarray:
    """astuv of the pixel centres along an axis of n pixels, as vertex/default.glsl's interpolation gives them in binary32"""
    return (((np.arange(n, dtype=F) + F(0.5))/F(n))*F(2) - F(1) + F(1))/F(2)


LOD_FRAGMENT = "void main() { fragColor = 0.5*textureLod(tex, astuv, 2.0) + 0.5*texture(tex, astuv*3.0); }"


def lod_scene(texels: np.ndarray, size: int = 32):
    from shaderflow_amd.scene import ShaderScene
    from shaderflow_amd.texture import ShaderTexture

    class Probe(ShaderScene):
        def build(self):
            texture = ShaderTexture(scene=self, name="tex", filter="linear", mipmaps=True)
            texture.from_numpy(np.flipud(texels))
            texture.repeat(True)
            self.shader.fragment = LOD_FRAGMENT

    scene = Probe()
    raw = scene.main(width=size, height=size, ssaa=1, subsample=1, fps=60.0, time=1/60, output=bytes)
    return np.frombuffer(raw, np.uint8).reshape(size, size, 3), scene


@pytest.mark.parametrize("tile", ["0", "tex"])
def test_texture_lod_through_the_python_api(monkeypatch, tile):
    """ShaderTexture(mipmaps=True) under `0.5*textureLod(tex, astuv, 2.0) + 0.5*texture(tex, astuv*3.0)`: the 32 x 32 frame is level 2
    (4 x 4) upsampled, plus the implicit lookup at the lambda of each pixel's OWN 2 x 2 quad (1.5 texels a pixel: levels 0 and 1
    blended), by the restatement, written as the unorm8 target writes it (x255, round half to even) — with the tile wished off and
    forced. The implicit half is the witness of the layout: a tiled code object's lanes walk rows, and drawn by it the differences
    would be between unrelated pixels and the picture another; the library has to send it to sfx_jit_render_quads."""
    monkeypatch.setenv("SHADERFLOW_JIT_TILE", tile)
    texels = T._data(16, 16, "rgba8")
    got, scene = lod_scene(texels)
    assert scene.shader.translated and ("#define SF_JIT_TILE_SLOT" in scene.shader._translation_text) == (tile == "tex")
    chain = O.build_mipmaps(O.make_texture(texels, "linear", True, True))
    reference = R.Texture([texels] + [O.mip_level(chain, k) for k in range(1, chain.levels)], "linear", True, True, True)
    centre = pixel_centres(32)
    moved = centre*F(3.0)
    uv = np.stack(np.meshgrid(moved, moved), axis=-1).astype(F)
    lam = T.quad_lambda(uv, (16, 16))
    assert 0.5 < float(lam.min()) and float(lam.max()) < 0.7                                 # log2(1.5): a blend of levels 0 and 1
    want, explicit_only = np.zeros((32, 32, 3), np.uint8), np.zeros((32, 32, 3), np.uint8)
    for j in range(32):
        for i in range(32):
            a = reference.at_lambda((float(centre[i]), float(centre[j])), 2.0)
            b = reference.at_lambda((float(moved[i]), float(moved[j])), float(lam[j, i]))
            c = np.array([R.add(R.mul(0.5, a[k]), R.mul(0.5, b[k])) for k in range(3)], F)
            want[j, i] = np.rint(np.clip(c, 0, 1)*F(255))
            flat = reference.at_level(0, (float(moved[i]), float(moved[j])))
            explicit_only[j, i] = np.rint(np.clip(np.array([R.add(R.mul(0.5, a[k]), R.mul(0.5, flat[k])) for k in range(3)], F), 0, 1)*F(255))
    assert np.array_equal(got, want), np.abs(got.astype(int) - want.astype(int)).max()
    assert not np.array_equal(want, explicit_only)                                           # … and the level of the implicit half shows


GLOW_UNIFORMS = [("sampler2D", "background")]


def glow_frames(cls, picture: np.ndarray, frames: int = 4) -> np.ndarray:
    from examples.scenes import make
    scene = make(cls, background=picture)
    raw = scene.main(width=96, height=54, fps=60.0, time=frames/60, ssaa=1, subsample=1, output=bytes)
    assert scene.shader.translated and not scene.shader.fallback, scene.shader.compile_error
    return np.frombuffer(raw, np.uint8).reshape(frames, 54, 96, 3)


def glow_on_the_host(picture: np.ndarray, frames: int = 4) -> np.ndarray:
    """the x86 host build of Glow's fragment over the same picture (chain: the oracle's, whose bytes the device's chain kernel is
    held to) at the clock's iTime of each frame"""
    from examples.scenes import Glow
    host = host_fragment(Glow.FRAGMENT, GLOW_UNIFORMS)
    times, _, _ = O.clock(60.0, frames)
    out = []
    for k in range(frames):
        host.set_uniforms(O.default_uniforms(96, 54, iTime=float(times[k])))
        host._keep.clear()
        host.bind_chain("background", np.flipud(picture), "linear", True, True)
        out.append(host.render(96, 54)[..., :3])
    return np.stack(out)


def test_glow_example_equals_the_host_build():
    """examples/scenes.py::Glow, 4 frames at 96 x 54, against the host build's frames for the same uniforms, byte for byte. The host
    build has no quad: its `textureOffset` taps on the chained background read level 0, while the device takes their level from the
    quad's differences (the example's own 640 x 360 picture under 96 x 54 pixels: lambda 2.7). So the comparison runs where the two
    must agree — a 48 x 27 picture, magnified (lambda = -1: level 0 on the device too) — and witnesses both halves of the example:
    levels 1 … 5 of the device-built chain through textureLod, and the nine offsets. The minified case is the next test's."""
    from examples.scenes import Glow
    from shaderflow_amd import synth
    picture = synth.background_image(48, 27, seed=3)
    got, want = glow_frames(Glow, picture), glow_on_the_host(picture)
    for k in range(4):
        assert np.array_equal(got[k], want[k]), (k, np.abs(got[k].astype(int) - want[k].astype(int)).max())
    assert got.std() > 10 and not np.array_equal(got[0], got[-1])                            # a picture, and it moves with iTime


def test_glow_minified_takes_its_offsets_at_the_implicit_level():
    """Glow over a 256 x 128 picture at 96 x 54 (lambda about 1.4, power-of-two extents: scaling by them is exact). Its sampler gets
    the LDS tile and its texture a chain, so the draw has to go to the untiled twin in the quad layout; the frames equal, byte for
    byte, those of the same fragment with every `textureOffset(background, astuv, o)` written as `textureGradOffset(background, astuv,
    dFdx(astuv), dFdy(astuv), o)` — the explicit form the probes hold to the host build and the restatement — and differ from the
    host build's, which reads those taps at level 0. Also the example as shipped (its own 640 x 360 picture) draws and moves."""
    from examples.scenes import Glow
    from shaderflow_amd import glsl2hip as G
    from shaderflow_amd import synth
    assert G.translate(Glow.FRAGMENT, GLOW_UNIFORMS).tiled_sampler == "background"
    tap = "textureOffset(background, astuv, ivec2(x, y))"
    assert Glow.FRAGMENT.count(tap) == 1

    class Explicit(Glow):
        FRAGMENT = Glow.FRAGMENT.replace(tap, "textureGradOffset(background, astuv, dFdx(astuv), dFdy(astuv), ivec2(x, y))")

    picture = synth.background_image(256, 128, seed=4)
    got, twin = glow_frames(Glow, picture, 2), glow_frames(Explicit, picture, 2)
    assert np.array_equal(got, twin), np.abs(got.astype(int) - twin.astype(int)).max()
    assert not np.array_equal(got, glow_on_the_host(picture, 2))
    shipped = glow_frames(Glow, None)
    assert shipped.std() > 10 and not np.array_equal(shipped[0], shipped[-1])
