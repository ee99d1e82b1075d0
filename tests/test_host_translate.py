"""
glsl2hip on the CPU: what the translator rewrites (and what it refuses), the bindings it hands to sfx_program_load, that its
output compiles for gfx950 (hipcc cross-compiles without a GPU), and the GLSL semantics of csrc/jit_runtime.hpp executed on
the host. The rendering of translated fragments is checked on the GPU (tests/test_gpu_translated.py).
"""
import re
import subprocess
from pathlib import Path

import pytest

from shaderflow_amd import glsl2hip as G

ROOT = Path(__file__).resolve().parent.parent
FRAGMENTS = ROOT/"tests"/"golden"/"jit"
CACHE = ROOT/"build"/"jit"


def body(cpp: str) -> str:
    return cpp.split("// ---- translated fragment ----")[1].split("// ---- end of translated fragment ----")[0]


def test_floating_literals_get_a_suffix_and_integers_do_not():
    out = body(G.translate("void main() { float a = 1.0 + .5 + 2. + 1e-4 + 3E5 + 7 + 0x1F + 2u + 1.5f + 4.0lf; }").cpp)
    assert "1.0f + .5f + 2.f + 1e-4f + 3E5f + 7 + 0x1F + 2u + 1.5f + 4.0f" in out
    assert G.translate("void main() { vec2 v1 = gluv; float b = v1.x*2.5; }").cpp.count("v1.x*2.5f") == 1     # `v1.x`: not a literal


def test_parameter_qualifiers_become_values_and_references():
    out = body(G.translate("void f(in float a, out vec3 b, inout float c, const in vec2 d) { b = vec3(a); c += d.x; }\nvoid main() {}").cpp)
    head = re.sub(r"\s+", " ", out.split("{")[0])
    assert "SF_HD void f(float a, vec3& b, float& c, const vec2 d)" in head
    assert "SF_HD void main_()" in out
    arrays = body(G.translate("float total(float values[3], const in vec2 pair[2]) { return values[0] + pair[1].x; }\n"
                              "void fill(out float values[3], inout vec2 p) { values[0] = p.x; }\nvoid main() {}").cpp)
    # arrays are values (csrc/jit_runtime.hpp sf_arr): an `in` array is the function's own copy, as in GLSL
    assert "SF_HD float total(sf_arr<float,3> values, const sf_arr<vec2,2> pair)" in arrays and "SF_HD void fill(sf_arr<float,3>& values, vec2& p)" in arrays


def test_declarations_of_the_engine_go_and_globals_become_members():
    source = """#version 330
    precision highp float;
    uniform float iLevel;
    uniform vec3 iShade = vec3(1);
    in vec2 stuv;
    layout(location = 0) out vec4 fragColor;
    in vec2 extra_varying;
    float helper(float x);
    float counter = 0;
    const float GAIN = 2.0*1.5;
    const int N = 3;
    const float SCALED = GAIN*N;
    const vec2 CORNER = vec2(1, 0);
    const float ROOT = sqrt(2.0);
    float helper(float x) { return x*GAIN; }
    void main() { fragColor = vec4(helper(iLevel)); }"""
    translation = G.translate(source)
    out = body(translation.cpp)
    assert "#version" not in out and "precision" not in out and "uniform" not in out and "layout" not in out
    assert "vec2 extra_varying;" in out and "in vec2" not in out
    assert out.count("helper") == 2                                             # the prototype is gone: definition and call remain
    assert "static constexpr float GAIN = 2.0f*1.5f;" in out and "static constexpr int N = 3;" in out and "static constexpr float SCALED = GAIN*N;" in out
    assert "const vec2 CORNER = vec2(1, 0);" in out and "static constexpr vec2" not in out
    assert "const float ROOT = sqrt(2.0f);" in out                             # a call: not a constant expression for C++
    assert "float counter = 0;" in out
    names = {(b.name, b.type, b.slot, b.count) for b in translation.bindings}
    assert names == {("iLevel", "float", 0, 1), ("iShade", "vec3", 1, 3)}
    assert "iLevel = user_(0);" in translation.cpp and "iShade = vec3(user_(1), user_(2), user_(3));" in translation.cpp


def test_bindings_follow_the_pipeline_and_skip_what_the_fragment_does_not_read():
    source = """#define background background0x0
    #define iScreen iScreen0x1
    #define iScreen1 iScreen1x1
    void main() { fragColor = texture(background, astuv)*iGain + texture(iSpectrogram, vec2(0, 0)) + float(iCount) + (iFlag ? 1 : 0) + iTime; }"""
    pipeline = [("float", "iTime"), ("sampler2D", "background0x0"), ("sampler2D", "iScreen0x1"), ("sampler2D", "iScreen1x1"), ("sampler2D", "iSpectrogram"),
                ("float", "iGain"), ("int", "iCount"), ("bool", "iFlag"), ("vec4", "iUnused"), ("sampler2D", "iWaveform")]
    translation = G.translate(source, pipeline)
    by_name = {b.name: b for b in translation.bindings}
    assert set(by_name) == {"background0x0", "iSpectrogram", "iGain", "iCount", "iFlag"}      # iScreen*: defined but not reached; iTime: built in
    assert by_name["iSpectrogram"].slot == 1 and by_name["background0x0"].slot == 0 and by_name["background0x0"].sampler
    assert (by_name["iGain"].slot, by_name["iCount"].slot, by_name["iFlag"].slot) == (0, 1, 2)
    assert by_name["iCount"].integer and by_name["iFlag"].integer and not by_name["iGain"].integer
    assert "iCount = user_int_(1);" in translation.cpp and "iFlag = user_int_(2) != 0;" in translation.cpp
    assert translation.cpp.rstrip().endswith("SF_JIT_ENTRY_POINTS(sf::rt::Fragment)") and "#undef background" in translation.cpp
    # the names a scene's pipeline really carries: `<name>0x0` boxes behind `#define <name> <name>0x0` keep the tape's slots too
    real = G.translate("#define iSpectrogram iSpectrogram0x0\n#define iWaveform iWaveform0x0\nvoid main() { fragColor = texture(iSpectrogram, astuv) + texture(iWaveform, astuv); }",
                       [("sampler2D", "iWaveform0x0"), ("sampler2D", "iSpectrogram0x0")])
    assert {b.name: b.slot for b in real.bindings} == {"iSpectrogram0x0": 1, "iWaveform0x0": 2}
    matrix = G.translate("uniform mat3 iMatrix;\nvoid main() { fragColor = vec4(iMatrix[0], 1); }")
    assert [(b.name, b.slot, b.count) for b in matrix.bindings] == [("iMatrix", 0, 9)] and "iMatrix = mat3(user_(0), " in matrix.cpp
    with pytest.raises(G.TranslationError):                                        # 17 x 4 floats: more than the 64-float uniform block
        G.translate("uniform vec4 weights[17];\nvoid main() { fragColor = weights[0]; }")
    with pytest.raises(G.TranslationError):
        G.translate("void main() { fragColor = " + " + ".join(f"texture(s{k}, stuv)" for k in range(17)) + "; }", [("sampler2D", f"s{k}") for k in range(17)])


def test_arrays_casts_keywords_and_discard():
    source = """
    const float WEIGHTS[] = float[](0.25, 0.5, 0.25);
    vec3[2] PAIR = vec3[2](vec3(0), vec3(1));
    struct Ray { vec3 origin; vec3 direction; };
    float new = 1.0;
    void main() {
        float taps[3] = float[3](1.0, 2.0, 3.0);
        int index = int(fragCoord.x) % 3;
        uint bits = uint(index) << 2u;
        Ray ray = Ray(vec3(0), vec3(0, 0, 1));
        bool not = false;
        if (taps[index] > 2.5 || not) discard;
        fragColor = vec4(WEIGHTS[index]*new + float(bits), PAIR[1].xy, ray.direction.z);
    }"""
    out = body(G.translate(source).cpp)
    out = re.sub(r" +", " ", out)
    assert "const sf_arr<float,3> WEIGHTS = sf_arr_of<float>(0.25f, 0.5f, 0.25f);" in out
    assert "sf_arr<vec3,2> PAIR = sf_arr_of<vec3>(vec3(0), vec3(1));" in out
    assert "sf_arr<float,3> taps = sf_arr_of<float>(1.0f, 2.0f, 3.0f);" in out
    assert "to_int(fragCoord.x) % 3" in out and "to_uint(index) << 2u" in out and "float(bits)" in out
    assert "float new_ = 1.0f;" in out and "bool not_ = false;" in out and "WEIGHTS[index]*new_" in out
    assert "{ discarded_ = true; return; }" in out
    assert "Ray ray = Ray(vec3(0), vec3(0, 0, 1));" in out                     # C++20 initialises the aggregate from parentheses
    assert "{ discarded_ = true; return {}; }" in G.translate("float f() { discard; return 1.0; }\nvoid main() {}").cpp
    with pytest.raises(G.TranslationError):
        G.translate("void main() { fragColor = vec4(0); ")


def test_operators_and_methods_c_plus_plus_does_not_have():
    out = body(G.translate("const float W[3] = float[3](1.0, 2.0, 3.0);\nvoid main() { bool a = stuv.x > 0.5 ^^ stuv.y > 0.5; float s = 0.0;\n"
                           "for (int i = 0; i < W.length(); i++) s += W[i]; fragColor = vec4(a ? s : float(fragColor.length ( ))); }").cpp)
    assert "stuv.x > 0.5f != stuv.y > 0.5f" in out and "i < length_of(W);" in out and "float(length_of(fragColor))" in out
    assert "length(p)" in body(G.translate("void main() { vec2 p = stuv; fragColor = vec4(length(p)); }").cpp)          # the function is left alone
    assert "(a && b) != c" in G.translate("void main() { bool a = true, b = false, c = true; fragColor = vec4(float((a && b) ^^ c)); }").cpp
    with pytest.raises(G.TranslationError):                                        # C++ has no operator between && and ||
        G.translate("void main() { bool a = true, b = false, c = true; fragColor = vec4(float(a && b ^^ c)); }")


UNIFORM_OPTIONS = """
const int TAPS = 3;
uniform float gain = 0.5;
uniform vec3 tint = vec3(1.0, 0.5, 0.25);
uniform vec2 both = vec2(2);
uniform int steps = 3;
uniform bool enabled = true;
uniform float weights[TAPS] = float[](0.25, 0.5, 0.125);
uniform vec2 offsets[2];
void main() {
    float total = 0;
    for (int k = 0; k < TAPS; k++) total += weights[k];
    fragColor = vec4(tint*gain*both.x, total + offsets[1].y + float(steps) + (enabled ? 0.0625 : 0));
}
"""


def test_uniform_initialisers_and_uniform_arrays():
    """GLSL 3.30 §4.3.5: `uniform float gain = 0.5;` reads 0.5 until the host sets it; `uniform T a[N]` is bound element by element"""
    translation = G.translate(UNIFORM_OPTIONS)
    by_name = {b.name: b for b in translation.bindings}
    assert by_name["gain"].default == (0.5,) and by_name["tint"].default == (1.0, 0.5, 0.25) and by_name["both"].default == (2.0, 2.0)
    assert by_name["steps"].default == (3.0,) and by_name["steps"].integer and by_name["enabled"].default == (1.0,)
    assert [by_name[f"weights[{k}]"].default for k in range(3)] == [(0.25,), (0.5,), (0.125,)] and by_name["weights[2]"].array == "weights"
    assert by_name["offsets[1]"].default is None and by_name["offsets[1]"].count == 2 and by_name["offsets[1]"].slot == by_name["offsets[0]"].slot + 2
    assert "sf_arr<float,3> weights;" in translation.cpp and "sf_arr<vec2,2> offsets;" in translation.cpp
    for bad in ("uniform float g = sqrt(2.0);\nvoid main() {}", "uniform float w[2] = float[](1.0);\nvoid main() {}",
                "uniform vec3 t = 1.0;\nvoid main() {}", "uniform float m[2][2];\nvoid main() {}"):
        with pytest.raises(G.TranslationError):
            G.translate(bad)


def test_uniform_initialisers_and_arrays_run_on_the_host():
    import numpy as np

    from tests.jit_host import HostFragment
    host = HostFragment(G.translate(UNIFORM_OPTIONS), CACHE)
    pixel = host.render_float(2, 2)[0, 0]
    assert np.allclose(pixel, [1.0, 0.5, 0.25, 0.875 + 0.0 + 3.0 + 0.0625])            # initialisers only; offsets[] starts as zeros
    host.set("gain", 1.0)
    host.set("offsets", [[0.0, 0.0], [0.0, 8.0]])
    host.set("weights", [1.0, 2.0, 3.0])
    host.set("enabled", 0)
    pixel = host.render_float(2, 2)[0, 0]
    assert np.allclose(pixel, [2.0, 1.0, 0.5, 6.0 + 8.0 + 3.0])


def test_fragments_that_take_derivatives_ask_for_the_quad_layout():
    assert "#define SF_JIT_DERIVATIVES 1" in G.translate("void main() { fragColor = vec4(fwidth(stuv.x)); }").cpp
    assert "#define SF_JIT_DERIVATIVES 1" in G.translate("#define slope(v) dFdx(v)\nvoid main() { fragColor = vec4(slope(stuv.x)); }").cpp
    assert "#define SF_JIT_DERIVATIVES 0" in G.translate("void main() { fragColor = vec4(stuv.x); }").cpp


def test_macros_are_rewritten_too_and_removed_afterwards():
    translation = G.translate("#define HALF 0.5\n#define scale(x) ((x)*2.0)\n#if 1\nvoid main() { fragColor = vec4(scale(HALF)); }\n#endif\n")
    assert "#define HALF 0.5f" in translation.cpp and "#define scale(x) ((x)*2.0f)" in translation.cpp
    assert "#undef HALF" in translation.cpp and "#undef scale" in translation.cpp and "#if 1" in translation.cpp


@pytest.mark.parametrize("name", sorted(p.stem for p in FRAGMENTS.glob("*.glsl")))
def test_repository_fragments_translate(name):
    translation = G.translate((FRAGMENTS/f"{name}.glsl").read_text(), [("sampler2D", "background")])
    assert "SF_HD void main_()" in translation.cpp
    assert translation.key == G.translate((FRAGMENTS/f"{name}.glsl").read_text(), [("sampler2D", "background")]).key


def test_translation_compiles_for_gfx950_and_exports_the_entry_points():
    translation = G.translate((FRAGMENTS/"polar.glsl").read_text())
    code = G.compile(translation, cache=CACHE)
    assert code.startswith((b"__CLANG_OFFLOAD_BUNDLE__", b"\x7fELF")) and b"gfx950" in code
    for symbol in (b"sfx_jit_render", b"sfx_jit_fused_1", b"sfx_jit_fused_2", b"sfx_jit_fused_4", b"sfx_jit_layout"):
        assert symbol in code, symbol
    assert (CACHE/f"{translation.key}.hsaco").exists()                         # second call: served from the cache
    assert G.compile(translation, cache=CACHE) == code


def test_compile_errors_carry_the_compiler_message():
    translation = G.translate("void main() { fragColor = undeclared_function(stuv); }")
    with pytest.raises(G.CompileError) as error:
        G.compile(translation, cache=CACHE)
    assert "undeclared_function" in str(error.value)


def test_runtime_header_semantics_on_the_host(tmp_path):
    """tests/jit_runtime_check.hip: swizzles, constructors, implicit conversions, matrix products and the prelude, run on the CPU"""
    binary = tmp_path/"jit_runtime_check"
    build = subprocess.run([G.HIPCC, "--offload-arch=gfx950", "-std=c++20", "-ffp-contract=off", "-O1", f"-I{G.CSRC}",
                            str(ROOT/"tests"/"jit_runtime_check.hip"), "-o", str(binary)], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(binary)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr


# ---- translated fragments executed on the host ---------------------------------------------------------------------------

def test_translated_fragments_on_the_host_match_the_opengl_goldens():
    """The repository's own fragments, translated and run on the CPU, against their OpenGL ES renderings (tests/golden/jit.npz)"""
    import json

    import numpy as np

    from oracle import binding as O
    from tests.jit_host import HostFragment
    golden = np.load(ROOT/"tests"/"golden"/"jit.npz")
    cases = json.loads(str(golden["cases"]))
    for name in ("waves", "cells", "hash", "builtins", "materials", "polar"):
        case = cases[name]
        host = HostFragment(G.translate((FRAGMENTS/f"{name}.glsl").read_text(), [("sampler2D", "background")]), CACHE)
        overrides = {k: (tuple(v) if isinstance(v, list) else v) for k, v in case["uniforms"].items()}
        host.set_uniforms(O.default_uniforms(case["width"], case["height"], **overrides))
        for key, value in {**case["floats"], **case["integers"]}.items():
            host.set(key, value)
        host.bind("background", golden["background"])
        got = host.render(case["width"], case["height"])
        d = np.abs(got.astype(int) - golden[f"{name}.image"].astype(int))
        assert d.max() <= 1 and (d == 0).mean() >= 0.98, (name, int(d.max()), float((d == 0).mean()))


def test_the_translator_asks_for_a_tile_only_where_it_can_pay(monkeypatch):
    """glsl2hip._sampler_worth_a_tile: taps in a loop (or many written out) on one sampler → SF_JIT_TILE_SLOT; a single tap, a fragment
    that takes derivatives, or SHADERFLOW_JIT_TILE=0 → none; SHADERFLOW_JIT_TILE=<name> forces"""
    monkeypatch.delenv("SHADERFLOW_JIT_TILE", raising=False)
    blur = "void main() { vec4 s = vec4(0); for (int k = -3; k <= 3; k++) s += texture(background, astuv + vec2(k, 0)/256.0); fragColor = s/7.0; }"
    single = "void main() { fragColor = texture(background, astuv); }"
    edges = "void main() { vec4 s = vec4(0); for (int k = 0; k < 4; k++) s += texture(background, astuv + k*0.01); fragColor = s*fwidth(astuv.x); }"
    two = ("uniform sampler2D other;\nvoid main() { vec4 s = texture(other, astuv); for (int k = 0; k < 4; k++) s += gtexture(background, gluv*0.5 + k*0.01) "
           "+ texture(other, stuv); fragColor = s; }")
    variables = [("sampler2D", "background")]
    t = G.translate(blur, variables)
    assert t.tiled_sampler == "background" and "#define SF_JIT_TILE_SLOT" in t.cpp
    slot = next(b.slot for b in t.bindings if b.name == "background")
    assert f"#define SF_JIT_TILE_SLOT {slot} " in t.cpp
    assert G.translate(single, variables).tiled_sampler is None
    assert G.translate(edges, variables).tiled_sampler is None
    after = "void main() { float a = 0; for (int k = 0; k < 4; k++) { a += k; } fragColor = a*texture(background, stuv); }"
    assert G.translate(after, variables).tiled_sampler is None           # a loop elsewhere in the text does not make one tap many
    braceless = "void main() { vec4 s = vec4(0); int k = 0; while (k < 4) s += texture(background, astuv + 0.01*k++); fragColor = s; }"
    assert G.translate(braceless, variables).tiled_sampler == "background"
    # helper functions tapping a sampler parameter: the taps count for the sampler a call passes, more when the call is in a loop
    helper = "vec4 blur(sampler2D tex, vec2 uv) { vec4 s = vec4(0); for (int k = -3; k <= 3; k++) s += texture(tex, uv + vec2(k, 0)/64.0); return s/7.0; }\n"
    once = "vec4 one(sampler2D tex, vec2 uv) { return texture(tex, uv); }\n"
    assert G.translate(helper + "void main() { fragColor = blur(background, astuv); }", variables).tiled_sampler == "background"
    assert G.translate(once + "void main() { fragColor = one(background, astuv) + one(background, stuv); }", variables).tiled_sampler is None
    assert G.translate(once + "void main() { vec4 s = vec4(0); for (int k = 0; k < 9; k++) { s += one(background, stuv + 0.01*k); } fragColor = s; }",
                       variables).tiled_sampler == "background"
    assert "SF_JIT_TILE_SLOT" not in G.translate(single, variables).cpp
    assert G.translate(two, variables).tiled_sampler in ("background", "other")
    monkeypatch.setenv("SHADERFLOW_JIT_TILE", "0")
    assert G.translate(blur, variables).tiled_sampler is None
    monkeypatch.setenv("SHADERFLOW_JIT_TILE", "background")
    assert G.translate(single, variables).tiled_sampler == "background"
    assert G.translate(edges, variables).tiled_sampler is None         # derivatives win over the wish


def test_host_build_of_a_tiled_translation_is_the_untiled_fragment(tmp_path, monkeypatch):
    """The tile exists on the device only; the host build of the same unit must compile and shade exactly what the untiled text shades"""
    import numpy as np

    from oracle import binding as O
    from tests.jit_host import HostFragment
    text = "void main() { vec4 s = vec4(0); for (int k = -3; k <= 3; k++) s += texture(background, astuv + vec2(k, k)/64.0); fragColor = s/7.0; }"
    data = np.random.default_rng(3).integers(0, 256, (24, 32, 4), dtype=np.uint8)
    images = []
    for tile in ("1", "0"):
        monkeypatch.setenv("SHADERFLOW_JIT_TILE", tile)
        translation = G.translate(text, [("sampler2D", "background")])
        assert (translation.tiled_sampler is not None) == (tile == "1")
        host = HostFragment(translation, CACHE)
        host.set_uniforms(O.default_uniforms(40, 20))
        host.bind("background", data, "linear", True, False)
        images.append(host.render_float(40, 20))
    assert np.array_equal(images[0].view(np.uint32), images[1].view(np.uint32))
