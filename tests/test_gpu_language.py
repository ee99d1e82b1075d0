"""
The GLSL 3.30 language rules of translated fragments ON THE DEVICE: the probes of tests/language_cases.py, translated and compiled for
gfx950 the way every fragment outside the registry is, drawn into an RGBA32F target of 4 x 4 group by group. Every row must equal the
specification's values and the x86 host build's bits (tests/test_host_language.py). The per-invocation fragments — a mutable global, a
checkerboard of discards — go through every entry point a code object exports: sfx_jit_render, the fused kernels at 1x, 2x and 4x
supersampling (a lane runs the fragment up to sixteen times there), and, with the LDS tile forced for a sampler that adds nothing,
the tiled forms of those (one more run of the fragment per block) and the quad-layout twin sfx_jit_render_quads.

Those draws are 130 x 8 pixels: two full blocks of 64 columns and a partial one.
"""
import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import _native as N
from tests import language_cases as L
from tests.helpers import Gpu
from tests.test_gpu_translated import load
from tests.test_host_language import host_fragment, host_results

pytestmark = pytest.mark.gpu
WIDTH, HEIGHT = 130, 8
FUSED = ((1, 1), (2, 2), (2, 1), (4, 4), (4, 2))          # (supersampling, subsample): sfx_jit_fused_1, _2, _2, _4, _4


@pytest.fixture(scope="module")
def gpu():
    g = Gpu()
    yield g
    g.close()


@pytest.fixture(scope="module")
def device(gpu):
    """probe -> {row: (4, 4, 4) float32} from the gfx950 code object; each probe is compiled and drawn once"""
    programs, done = [], {}

    def results(probe):
        if probe not in done:
            prog, _ = load(gpu, L.probe_glsl(probe))
            programs.append(prog)
            gpu.set_uniforms(prog, O.default_uniforms(*L.SIZE))
            assert gpu.set_values(prog, "two", 2, integer=True)
            target = gpu.empty(*L.SIZE, 4, np.float32)

            def render(group):
                assert gpu.set_values(prog, "group", group, integer=True)
                N.check(gpu.lib.sfx_render(prog, target, 0))
                return gpu.read(target, *L.SIZE, 4, np.float32)
            done[probe] = L.evaluate(probe, render)
        return done[probe]
    yield results
    for prog in programs:
        N.check(gpu.lib.sfx_program_destroy(prog))


@pytest.mark.parametrize("probe", L.PROBES)
def test_device_rows_compute_what_glsl_computes(device, probe):
    L.check(probe, device(probe))


@pytest.mark.parametrize("probe", L.PROBES)
def test_device_equals_the_host_build_bit_for_bit(device, probe):
    L.check_same(probe, device(probe), host_results(probe), "device against the x86 host build")


# ---- every entry point, once per invocation -----------------------------------------------------------------------------------------
def mipmapped(gpu: Gpu) -> N.Handle:
    texels = np.random.default_rng(3).integers(0, 256, (16, 16, 4), dtype=np.uint8)
    handle = gpu.texture(texels, "linear", True, True)
    N.check(gpu.lib.sfx_texture_build_mipmaps(handle))
    N.check(gpu.lib.sfx_texture_params(handle, 2, 1, 1))        # FILTER_LINEAR_MIPMAP: the unfused draw takes the quad layout
    return handle


def entry_points(gpu: Gpu, name: str, monkeypatch) -> dict:
    """{entry point: frame} of the fragment: "render" (130 x 8 x 4 float32), ("fused", ssaa, subsample) and ("two pass", ssaa, subsample)
    (130 x 8 x 3 bytes: sfx_render at 130*ssaa x 8*ssaa into the RGBA8 screen, then sfx_resolve; ("screen", …) is that draw into a
    float target), and for the tapped fragment "quads": the
    unfused draw with a mipmapped texture bound, which a tiled code object hands to its twin"""
    tapped = name == "tapped"
    monkeypatch.setenv("SHADERFLOW_JIT_TILE", "tex" if tapped else "0")
    prog, translation = load(gpu, L.PER_INVOCATION[name], [("sampler2D", "tex")])
    assert (translation.tiled_sampler == "tex") == tapped and ("#define SF_JIT_TILE_SLOT" in translation.cpp) == tapped
    assert [gpu.lib.sfx_program_fusable(prog, ssaa) for ssaa in (1, 2, 4)] == [1, 1, 1]
    if tapped:
        plain = np.random.default_rng(4).integers(0, 256, (9, 7, 4), dtype=np.uint8)
        assert gpu.bind(prog, "tex", gpu.texture(plain, "linear", True, False))
    frames = {}
    gpu.set_uniforms(prog, O.default_uniforms(WIDTH, HEIGHT))
    frames["render"] = gpu.render(prog, WIDTH, HEIGHT, comps=4, dtype=np.float32)
    for (ssaa, subsample) in FUSED:
        gpu.set_uniforms(prog, O.default_uniforms(WIDTH*ssaa, HEIGHT*ssaa, iSSAA=float(ssaa)))      # iResolution counts samples: gl_FragCoord is a sample's
        frames["fused", ssaa, subsample] = gpu.render_resolve(prog, WIDTH, HEIGHT, ssaa, subsample)
        frames["screen", ssaa, subsample] = gpu.render(prog, WIDTH*ssaa, HEIGHT*ssaa, comps=4, dtype=np.float32)
        frames["two pass", ssaa, subsample] = gpu.resolve(gpu.render(prog, WIDTH*ssaa, HEIGHT*ssaa), WIDTH, HEIGHT, subsample)
    if tapped:
        assert gpu.bind(prog, "tex", mipmapped(gpu))
        gpu.set_uniforms(prog, O.default_uniforms(WIDTH, HEIGHT))
        frames["quads"] = gpu.render(prog, WIDTH, HEIGHT, comps=4, dtype=np.float32)
    N.check(gpu.lib.sfx_program_destroy(prog))
    return frames


def test_a_mutable_global_starts_over_in_every_invocation(gpu, monkeypatch):
    """`float seen = 1.0; void main(){ seen += 1.0; fragColor = vec4(seen/4.0); }` is 0.5 in every sample of every entry point: a
    fragment object reused between the invocations of a lane would give 0.75, 1.0, …"""
    frames = entry_points(gpu, "seen", monkeypatch)
    for key, frame in frames.items():
        if frame.dtype == np.float32:
            assert (frame == 0.5).all(), (key, np.unique(frame)[:8])
        else:                                                         # bytes: 127.5 rounds to 128 to even and half up alike
            assert (frame == 128).all(), (key, np.unique(frame)[:8])
    assert set(frames) >= {"render", ("fused", 1, 1), ("fused", 2, 2), ("fused", 4, 4)}


@pytest.mark.parametrize("name", ["checker", "tapped"])
def test_a_checkerboard_of_discards_on_every_entry_point(gpu, monkeypatch, name):
    """every other sample is discarded: the unfused draws hold the colour where x + y is even and zeros elsewhere (the host build's
    bits), and every fused kernel gives, byte for byte, the mean that the unfused render followed by sfx_resolve gives. "tapped" also
    counts its invocations (a kept sample is the colour times seen/2 = 1) on the tiled kernels and on the quad-layout twin"""
    frames = entry_points(gpu, name, monkeypatch)

    def board(width, height):
        y, x = np.mgrid[0:height, 0:width]
        return np.where((((x + y) & 1) == 0)[..., None], np.array(L.KEPT, np.float32), np.float32(0)).astype(np.float32)
    for key in [k for k in frames if k == "render" or k == "quads" or k[0] == "screen"]:
        ssaa = 1 if isinstance(key, str) else key[1]
        assert np.array_equal(frames[key], board(WIDTH*ssaa, HEIGHT*ssaa)), key
    assert ("quads" in frames) == (name == "tapped")
    if name == "checker":
        host = host_fragment(name)
        host.set_uniforms(O.default_uniforms(WIDTH, HEIGHT))
        assert np.array_equal(frames["render"].view(np.uint32), host.render_float(WIDTH, HEIGHT).view(np.uint32))
    for (ssaa, subsample) in FUSED:
        fused, two_pass = frames["fused", ssaa, subsample], frames["two pass", ssaa, subsample]
        assert np.array_equal(fused, two_pass), ((ssaa, subsample), np.abs(fused.astype(int) - two_pass.astype(int)).max())
        assert fused.std() > 0 or ssaa > 1                              # 1x keeps the board; above, every pixel averages kept and discarded samples
    assert 0 < frames["fused", 2, 2].mean() < 255*0.75
