"""
The GLSL 3.30 §8.7 texture lookups of translated fragments (csrc/jit_runtime.hpp on csrc/glsl.hpp's "THE RULES") on the CPU: the
probes of tests/texture_cases.py built for the x86 host (tests/texture_host.py) against the exact-arithmetic restatement
tests/texture_ref.py, bit for bit. The host build has no quad (glsl.hpp quad_dx returns 0), so it witnesses every EXPLICIT form —
lod, gradients, offsets, fetches, sizes, projection; bias and implicit derivatives are tests/test_gpu_texture.py's.
"""
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import glsl2hip as G
from tests import texture_cases as T
from tests import texture_ref as R
from tests.texture_host import TextureHostFragment, packed_offsets

ROOT = Path(__file__).resolve().parent.parent
CACHE = ROOT/"build"/"jit"
F = np.float32
PROBES = {"explicit": T.EXPLICIT_FORMS, "proj": T.PROJ_FORMS}


@lru_cache(maxsize=None)
def host_probe(probe: str) -> TextureHostFragment:
    host = TextureHostFragment(G.translate(T.probe_glsl(PROBES[probe]), T.PROBE_UNIFORMS), CACHE)
    host.set_uniforms(O.default_uniforms(T.WIDTH, T.HEIGHT))
    return host


def host_run(probe: str, config: T.Config, form: int, operands: np.ndarray, gradients: np.ndarray, data=None) -> np.ndarray:
    host = host_probe(probe)
    host._keep.clear()
    if config.chain:
        host.bind_chain("tex", config.data, config.filter, config.repeat_x, config.repeat_y)
    else:
        assert host.bind("tex", config.data if data is None else data, config.filter, config.repeat_x, config.repeat_y)
    assert host.bind("operands", operands, "nearest", False, False) and host.bind("gradients", gradients, "nearest", False, False)
    host.set("form", form)
    return host.render_float(T.WIDTH, T.HEIGHT).reshape(T.ROWS, 4)


@lru_cache(maxsize=None)
def host_results(probe: str) -> dict:
    return T.evaluate(host_run, probe, PROBES[probe])


@pytest.fixture(scope="module")
def explicit():
    return host_results("explicit")


def test_the_table_has_the_whole_sampler2d_column_and_every_shape():
    wanted = ("textureSize texture textureProj textureLod textureOffset texelFetch texelFetchOffset textureProjOffset textureLodOffset "
              "textureProjLod textureProjLodOffset textureGrad textureGradOffset textureProjGrad textureProjGradOffset").split()
    probed = {name.partition("@")[0].rstrip("34") for name in (*T.EXPLICIT_FORMS, *T.PROJ_FORMS)}
    assert set(wanted) <= probed, set(wanted) - probed
    header = (G.CSRC/"jit_runtime.hpp").read_text()
    for name in wanted:
        assert f" {name}(sampler2D s" in header, name
    for size in T.SIZES:                                              # every size: every format, wrap pair and filter / chain mode
        mine = [c for c in T.CONFIGS if (c.width, c.height) == size]
        assert {c.format for c in mine} == set(T.FORMATS) and {(c.repeat_x, c.repeat_y) for c in mine} == set(T.WRAPS)
        assert {(c.filter, c.chain) for c in mine} == set(T.MODES)
    assert {((c.repeat_x, c.repeat_y), (c.filter, c.chain)) for c in T.CONFIGS} == {(w, m) for w in T.WRAPS for m in T.MODES}


def test_the_oracles_chain_is_packed_as_the_header_reads_it():
    for config in T.CONFIGS:
        if config.chain:
            texture = T.oracle_texture(config)
            texel_bytes = config.data.shape[2]*config.data.dtype.itemsize
            want = packed_offsets(config.width, config.height, texel_bytes, texture.levels)
            got = [O.lib().sfo_mip_offset(O.C.byref(texture), level) for level in range(1, texture.levels)]
            assert got == want and all(offset % 16 == 0 for offset in got), config.name


def test_the_restatement_equals_the_oracles_sampler_bit_for_bit():
    """texture_ref is itself pinned: at lod 0 without an offset it is O.sample on the texture, at an integer level d it is O.sample
    on that level as a texture of its own"""
    for config in T.CONFIGS:
        reference = T.reference(config)
        for level, texels in enumerate(reference.levels):
            oracle = O.make_texture(texels, config.filter, config.repeat_x, config.repeat_y)
            for uv in T.coordinates(config.width, config.height):
                want = O.sample(oracle, float(uv[0]), float(uv[1]))
                got = np.array(reference.at_lambda(uv, float(level)), F)      # (ceil(d + 0.5) - 1 = d: the nearest-level rule lands there too)
                assert np.array_equal(T.bits(got), T.bits(want)), (config.name, level, uv, got, want)


def test_rounding_to_binary32_is_numpys():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(400).astype(F), (rng.standard_normal(400)*rng.choice([1e-30, 1.0, 1e20], 400)).astype(F)
    for x, y in zip(a.tolist(), b.tolist()):
        assert T.bits(np.array([R.mul(x, y)], F))[0] == T.bits(np.array([F(x)*F(y)]))[0]
        assert T.bits(np.array([R.add(x, y)], F))[0] == T.bits(np.array([F(x) + F(y)]))[0]
    assert R.rn(R.Fraction(1, 3)) == float(F(1)/F(3)) and R.rn(R.Fraction(1, 2**149)) == 2.0**-149 and R.rn(R.Fraction(1, 2**150)) == 0.0
    assert R.rn(R.Fraction(2**24 + 1)) == 2.0**24 and R.rn(R.Fraction(2**24 + 3)) == 2.0**24 + 4      # ties to even


def test_operands_come_back_bit_for_bit(explicit):
    T.check_echo(explicit)


def test_every_explicit_form_equals_the_restatement_bit_for_bit(explicit):
    T.check_reference(explicit)


def test_every_projective_form_equals_its_twin_at_the_divided_coordinate(explicit):
    T.check_projective(host_run, explicit, host_results("proj"))


def test_offsets_are_rolls_and_lods_without_a_chain_select_nothing(explicit):
    T.check_identities(host_run, explicit)


def test_a_chain_under_a_plain_filter_is_not_sampled_but_can_be_fetched():
    """NEAREST / LINEAR with a chain attached: every lod and gradient reads level 0 (minification and magnification coincide), while
    texelFetch and textureSize see the levels"""
    config = next(c for c in T.CONFIGS if c.chain and c.format == "rgba8" and c.width == 8)
    plain = T.Config(**{**config.__dict__, "chain": False})
    host, forms = host_probe("explicit"), list(T.EXPLICIT_FORMS)
    for name in ("textureLod", "textureGrad", "textureLodOffset@2", "texelFetch", "textureSize"):
        rows = T.rows_of(config, name)                                # (the chained config's rows: lods up to its top + 3)
        host._keep.clear()
        host.bind_chain("tex", config.data, config.filter, config.repeat_x, config.repeat_y, mipmap=False)
        for sampler, texels in zip(("operands", "gradients"), T.operand_textures(rows)):
            assert host.bind(sampler, texels, "nearest", False, False)
        host.set("form", forms.index(name))
        got = host.render_float(T.WIDTH, T.HEIGHT).reshape(T.ROWS, 4)[:len(rows)]
        want = T.expected(config if name in ("texelFetch", "textureSize") else plain, name, rows)
        T.assert_same_bits(got, want, name)


def test_texture_lod_reads_the_level_it_names(explicit):
    """Fails on the parent commit (textureLod dropped its lod and read level 0): textureLod(s, uv, 2.0) on the mipmapped 8x8 is
    level 2's bilinear sample"""
    config = next(c for c in T.CONFIGS if c.chain and c.filter == "linear" and c.width == 8)
    level2 = O.make_texture(O.mip_level(T.oracle_texture(config), 2), "linear", config.repeat_x, config.repeat_y)
    table = T.rows_of(config, "textureLod").copy()
    table[:, 2] = 2.0
    got = host_run("explicit", config, list(T.EXPLICIT_FORMS).index("textureLod"), *T.operand_textures(table))[:len(table)]
    want = np.array([O.sample(level2, float(u), float(v)) for u, v in table[:, :2]], F)
    level0 = np.array([O.sample(O.make_texture(config.data, "linear", config.repeat_x, config.repeat_y), float(u), float(v)) for u, v in table[:, :2]], F)
    assert not np.array_equal(want, level0)
    T.assert_same_bits(got, want, "textureLod(s, uv, 2.0) against level 2")


@pytest.mark.parametrize("size", [(8, 8), (16, 4)])
def test_the_bias_probe_runs_through_every_level(size):
    """the coordinates of BIAS_GLSL (tests/test_gpu_texture.py runs it; the device's uv must equal this restatement) give a lambda_base
    from magnification through every pair of levels to beyond the top of both power-of-two textures"""
    lam = T.quad_lambda(T.bias_uv(), size)
    assert T.covers_every_level(lam, max(size).bit_length() - 1), (float(lam.min()), float(lam.max()))


def blur(tile: str, monkeypatch):
    monkeypatch.setenv("SHADERFLOW_JIT_TILE", tile)
    return G.translate(T.BLUR_GLSL, [("sampler2D", "tex")])


def test_the_offset_blur_compiles_and_gets_a_tile(monkeypatch):
    """Fails on the parent commit (textureOffset was undeclared: hipcc rejected the probe). The blur's taps count for the tile
    heuristic; on the host build the tile is never staged (JitShader<F> runs untiled), so what is checked here is the translation
    and the values — the same frame with the tile wished off and on; tests/test_gpu_texture.py compares the staged tile's frames"""
    untiled, tiled, default = blur("0", monkeypatch), blur("tex", monkeypatch), blur("1", monkeypatch)
    assert untiled.tiled_sampler is None and tiled.tiled_sampler == "tex" and default.tiled_sampler == "tex"
    assert "#define SF_JIT_TILE_SLOT" in tiled.cpp and "#define SF_JIT_TILE_SLOT" not in untiled.cpp
    config = next(c for c in T.CONFIGS if not c.chain and c.filter == "linear" and c.width == 8)
    frames = []
    for translation in (untiled, tiled):
        host = TextureHostFragment(translation, CACHE)
        host.set_uniforms(O.default_uniforms(T.WIDTH, T.HEIGHT))
        assert host.bind("tex", config.data, config.filter, config.repeat_x, config.repeat_y)
        frames.append(host.render_float(T.WIDTH, T.HEIGHT))
    assert np.array_equal(T.bits(frames[0]), T.bits(frames[1])) and frames[0].std() > 0.01
    # … and the frame is the sum the fragment writes, by the restatement
    reference = T.reference(config)
    reach = range(-T.BLUR_REACH, T.BLUR_REACH + 1)
    for (i, j) in ((0, 0), (7, 3), (15, 15)):
        astuv = (F(F(i) + F(0.5))/F(T.WIDTH), F(F(j) + F(0.5))/F(T.HEIGHT))
        astuv = tuple(float((F(2.0)*c - F(1.0) + F(1.0))/F(2.0)) for c in astuv)           # agluv = centre*2 - 1, astuv = (agluv + 1)/2
        uv = tuple(R.sub(R.mul(c, 1.25), 0.125) for c in astuv)
        total = [0.0]*4
        for x in reach:
            for y in reach:
                tap = reference.at_level(0, uv, (x, y))
                total = [R.add(total[k], tap[k]) for k in range(4)]
        want = np.array([R.rn(R.Fraction(t)/9) for t in total], F)
        assert np.array_equal(T.bits(frames[0][j, i]), T.bits(want)), ((i, j), frames[0][j, i], want)
