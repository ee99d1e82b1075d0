"""
The GLSL 3.30 language rules of translated fragments on the CPU: the probes of tests/language_cases.py built for the x86 host
(tests/jit_host.py) must give, row by row and exactly, the values the specification gives; the constructs the translator does not take
must be refused by name at translation time; and each rewrite the rows needed is held as text. tests/test_gpu_language.py holds the
gfx950 build to the same values and to this build's bits.
"""
import re

import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import glsl2hip as G
from tests import language_cases as L
from tests.jit_host import HostFragment
from tests.test_host_translate import CACHE, body

_results: dict = {}


def host_results(probe: str) -> dict:
    """{row: (4, 4, 4) float32} of the probe's host build; once per session"""
    if probe not in _results:
        host = HostFragment(G.translate(L.probe_glsl(probe)), CACHE)
        host.set_uniforms(O.default_uniforms(*L.SIZE))
        host.set("two", 2)

        def render(group):
            host.set("group", group)
            return host.render_float(*L.SIZE)
        _results[probe] = L.evaluate(probe, render)
    return _results[probe]


def host_fragment(name: str) -> HostFragment:
    host = HostFragment(G.translate(L.PER_INVOCATION[name]), CACHE)
    host.set_uniforms(O.default_uniforms(8, 8))
    return host


@pytest.mark.parametrize("probe", L.PROBES)
def test_every_row_computes_what_glsl_computes(probe):
    L.check(probe, host_results(probe))


def test_the_table_holds_the_constructs_it_was_written_for():
    names = " | ".join(L.BY_NAME)
    for wanted in ("T[n] a, b", "a == b and a != b", "assignment copies", "from int variables", "as a function argument", ".length() of a local, a global",
                   "`in` parameter written", "through function parameters", "of structs, and inside structs", "struct: constructor", "nested structs",
                   "`inout` parameter and return value", "struct: == and !=", "v.wzyx = v, a.zyx = a, b.yx = b", "v.xy = v.yx, v.yzw = v.xyz",
                   "w.xy += w.yx, u.zx *= u.xz", "m[1].xy = m[1].yx, m[0] = m[1]", "chained a = u.zw", "rgba and stpq", "on ivec and uvec",
                   "first component", "bool(2), bool(-0.5)", "bvec from ivec and vec", "truncation", "truncates toward zero", "diagonal, from ints, from columns",
                   "mat2(vec4)", "++ and -- on scalars", "++ and -- on vectors", "v *= m, m *= m, m*v, v*m", "a swizzle, matrices and bvec", "& | ^ ~", "<< >>",
                   "unary minus on uint", "int / float mixing", "wrap around", "const in, out, inout", "reads a global", "a swizzle and a matrix column",
                   "left to right", "do not evaluate their right side", "overloads", "prototypes, f(void)", "fall-through", "reuses the counter's name",
                   "early return", "discard in main", "discard inside a function", "chains of const", "non-constant initialiser", "named like built-in",
                   "C++ keywords", "#version", "literals", "backslash-newline", "__LINE__"):
        assert wanted in names, wanted
    assert {r.probe for r in L.ROWS} == set(L.PROBES) and len(L.PROBES) + len(L.PER_INVOCATION) <= 8      # code objects: hipcc takes seconds for each
    quoted = " ".join(r.body + r.helpers for r in L.ROWS) + " ".join(text for (_, _, text, _) in L.REFUSALS)
    for snippet in ("vec4 v=vec4(1,2,3,4); v.wzyx = v;", "vec3 a=vec3(1,2,3); a.zyx = a;", "vec2 b=vec2(1,2); b.yx = b;",
                    "float a[2]=float[2](1.,2.), b[2]=float[2](1.,2.);", "float b[3]; b = a;", "(float a[2]){a[0]=7.;", "v++; iv4++;",
                    "mat2 d = mat2(vec4(1,2,3,4));", "float f = float(d.zyx);", "float[2] p, q;", "int i=1,j=2; float w[2]=float[2](i,j);", "s.w.length()",
                    "float new=1.; float new_=2.;", "lessThan(a, vec3(2.)) == bvec3(true,false,false)", "lc_set(v.zw)"):
        assert snippet in quoted, snippet


@pytest.mark.parametrize("name,section,text,words", L.REFUSALS, ids=[r[0] for r in L.REFUSALS])
def test_what_is_not_taken_is_refused_by_name_at_translation_time(name, section, text, words):
    with pytest.raises(G.TranslationError) as refusal:
        G.translate(text)
    assert words in str(refusal.value), (name, section, str(refusal.value))


def test_per_invocation_fragments_on_the_host():
    """every invocation starts from the fragment's initialisers; a discarded one leaves zeros"""
    assert (host_fragment("seen").render_float(8, 8) == 0.5).all()
    got = host_fragment("checker").render_float(8, 8)
    y, x = np.mgrid[0:8, 0:8]
    kept = ((x + y) & 1) == 0
    assert (got[kept] == np.array([0.25, 0.5, 0.75, 1.0], np.float32)).all() and (got[~kept] == 0).all()


# ---- the rewrites behind the rows, as text ----------------------------------------------------------------------------------------
def translated(text: str) -> str:
    return re.sub(r"[ \t]+", " ", body(G.translate(text).cpp))


def test_arrays_are_declared_as_values():
    out = translated("struct S { float w[2]; };\nconst float W[] = float[](1., 2., 3.);\nfloat g[2], h;\n"
                     "float[2] mk(float a[2], out vec2 b[3], const in S s) { return a; }\n"
                     "void main() { float a[3] = float[3](1., 2., 3.), b[3], c = 1.; float[2] p, q; int n[] = int[](1, 2); }")
    assert "struct S { sf_arr<float,2> w;" in out and "const sf_arr<float,3> W = sf_arr_of<float>(1.f, 2.f, 3.f);" in out
    assert "sf_arr<float,2> g; float h;" in out
    assert "SF_HD sf_arr<float,2> mk(sf_arr<float,2> a, sf_arr<vec2,3>& b, const S s)" in out
    assert "sf_arr<float,3> a = sf_arr_of<float>(1.f, 2.f, 3.f), b; float c = 1.f;" in out
    assert "sf_arr<float,2> p, q;" in out and "sf_arr<int,2> n = sf_arr_of<int>(1, 2);" in out
    uniform = G.translate("uniform float w[2] = float[](1., 2.);\nfloat f(float v[2]) { return v[1]; }\nvoid main() { fragColor = vec4(f(w)); }")
    assert "sf_arr<float,2> w;" in uniform.cpp and [b.default for b in uniform.bindings] == [(1.0,), (2.0,)]      # a uniform array is such a value too


def test_length_of_takes_the_whole_postfix_expression():
    out = translated("struct S { float w[4]; };\nS many[2];\nvoid main() { S s; fragColor = vec4(s.w.length(), many[1].w.length(), many.length(), fragColor.xyz.length()); }")
    assert "vec4(length_of(s.w), length_of(many[1].w), length_of(many), length_of(fragColor.xyz))" in out


def test_structs_get_the_memberwise_comparison():
    out = translated("struct Ray { vec3 o; vec3 d; };\nvoid main() {}")
    assert "struct Ray { vec3 o; vec3 d; SF_HD bool operator==(const Ray&) const = default; };" in out


def test_a_swizzle_in_an_out_position_goes_through_sf_out():
    out = translated("void set(out vec2 p, float k) { p = vec2(k); }\nvoid both(inout vec2 p) { p *= 2.; }\n"
                     "void main() { vec4 v; vec2 u; set(v.zw, v.x); set(u, 1.); both(v.yx); float w = modf(v.x, v.y); vec2 f = modf(v.xy, v.zw); }")
    assert "set(sf_out(v.zw), v.x); set(u, 1.f); both(sf_out(v.yx)); float w = modf(v.x, v.y); vec2 f = modf(v.xy,sf_out( v.zw));" in out
    assert "SF_HD void set(vec2& p, float k)" in out                           # the definition is no call


def test_a_continued_define_is_one_line_and_lines_stay_the_fragments():
    cpp = G.translate("#define TWO \\\n    2.0\nfloat f() { return TWO; }\nvoid main() {\n#define K 1.0\n    fragColor = vec4(f() + K + float(__LINE__));\n}\n").cpp
    assert re.search(r"#define TWO +2\.0f\n", cpp)
    assert "SF_HD float f()\n#line 3\n{ return TWO; }" in cpp and "SF_HD void main_()\n#line 4\n{" in cpp and "#define K 1.0f\n#line 6\n" in cpp
