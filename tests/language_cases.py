"""
The GLSL 3.30 language rules of translated fragments (shaderflow_amd/glsl2hip.py + csrc/jit_runtime.hpp), row by row: what a fragment SAYS —
statements, operators, constructors, l-values, arrays, structs, parameter passing (§3-§6) — where tests/math_cases.py, vector_cases.py and
texture_cases.py hold what it CALLS. Shared by tests/test_host_language.py (x86 host build of the probes, CPU) and tests/test_gpu_language.py
(the gfx950 code objects of the same translations). No GPU and no pytest in here.

A row is a GLSL body that sets `vec4 r` (plus the globals, structs and functions it needs, prefixed `lc_` / `Lc` / `LC_`: rows share a
translation unit) and the four floats GLSL 3.30 gives, written down from the specification's section named in the row. Every operand is a
small integer or a dyadic fraction, so every expected value is exact in binary32 and every comparison is equality. Rows are grouped into a
few probes; `uniform int group` selects the row, `uniform int two` is 2 (a value the compiler cannot fold). A probe is drawn 4 x 4 and
every pixel must hold the row's values.

REFUSALS are valid GLSL that the translator does not take: `translate()` must raise TranslationError with the quoted words (nothing may
fail later, inside hipcc). PER_INVOCATION are two whole fragments for the kernels' entry points: a mutable global (a fragment object
reused between invocations would count up) and a checkerboard of discards.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F = np.float32


@dataclass
class Row:
    name: str
    section: str                              # GLSL 3.30 specification
    probe: str
    body: str                                 # sets `r`; or writes fragColor and returns / discards
    want: tuple                               # four floats
    helpers: str = ""                         # global scope: structs, globals, functions


ROWS: list[Row] = []


def row(probe: str, name: str, section: str, body: str, want: tuple, helpers: str = "") -> None:
    assert len(want) == 4 and all(float(F(v)) == float(v) for v in want), name      # exact in binary32
    ROWS.append(Row(name, section, probe, body.strip(), tuple(float(v) for v in want), helpers.strip()))


# ---- arrays (§4.1.9, §5.4.4, §5.8, §5.9) ----------------------------------------------------------------------------------------
row("aggregates", "array: sized, unsized and T[n] declarations, T[n] a, b", "4.1.9", """
    float a[3]; a[0] = 1.0; a[1] = 2.0; a[2] = 4.0;
    float b[] = float[](8.0, 16.0);
    float[2] c = float[2](32.0, 64.0);
    float[2] p, q; p[0] = 1.0; p[1] = 2.0; q = p; q[1] = 3.0;
    float d[2], e = 0.5, f[3];
    d[1] = 1.0; f[2] = 2.0;
    r = vec4(a[0] + a[1] + a[2], b[0] + b[1], c[0] + c[1] + e + d[1] + f[2], p[1]*10.0 + q[1] + float(q.length()) + float(f.length())*100.0);
""", (7, 24, 99.5, 325))
row("silent", "array: a == b and a != b compare the elements", "5.9", """
    float a[2]=float[2](1.,2.), b[2]=float[2](1.,2.);
    r.xy = vec2(lc_b(a==b), lc_b(a!=b));
    b[1] = 3.0;
    r.zw = vec2(lc_b(a==b), lc_b(a!=b));
""", (1, 0, 0, 1))
row("aggregates", "array: assignment copies, the source stays", "5.8", """
    float a[3] = float[3](1., 2., 3.);
    float b[3]; b = a;
    b[0] = 9.; a[2] = 7.;
    r = vec4(a[0], a[2], b[0], b[2]);
""", (1, 7, 9, 3))
row("aggregates", "array: constructor from int variables", "5.4.4", """
    int i=1,j=2; float w[2]=float[2](i,j);
    r = vec4(w[0], w[1], w[0]/w[1], float(w.length()));
""", (1, 2, 0.5, 2))
row("aggregates", "array: constructor as a function argument", "5.4.4", """
    r.x = lc_sum3(float[3](1., 2., 4.));
    r.y = lc_sum3(float[](8., 16., 32.));
""", (7, 56, 0, 0), "float lc_sum3(float v[3]) { return v[0] + v[1] + v[2]; }")
row("aggregates", "array: .length() of a local, a global, a parameter and a struct member", "4.1.9", """
    float a[2]; LcHold s;
    r = vec4(a.length(), lc_g5.length(), lc_len(float[3](1., 2., 3.)), s.w.length());
""", (2, 5, 3, 4), "float lc_g5[5];\nstruct LcHold { float w[4]; int n; };\nint lc_len(float v[3]) { return v.length(); }")
row("aggregates", "array: an `in` parameter written inside the function is a copy", "6.1.1", """
    float a[2] = float[2](1., 2.);
    float s = lc_first(a);
    r = vec4(s, a[0], a[1], 0.);
""", (9, 1, 2, 0), "float lc_first(float a[2]){a[0]=7.; return a[0] + a[1];}")
row("aggregates", "array: == and != through function parameters", "5.9", """
    float a[2] = float[2](1., 2.); float b[2] = float[2](1., 2.); float c[2] = float[2](1., 3.);
    r = vec4(lc_b(lc_same(a, b)), lc_b(lc_same(a, c)), lc_b(lc_differ(a, b)), lc_b(lc_differ(a, c)));
""", (1, 0, 0, 1), "bool lc_same(float a[2], float b[2]) { return a == b; }\nbool lc_differ(in float a[2], const in float b[2]) { return a != b; }")
row("aggregates", "array: of structs, and inside structs", "4.1.9", """
    LcP ps[2] = LcP[2](LcP(1.5, 2), LcP(2.5, 3));
    LcBag bag = LcBag(vec2[2](vec2(1., 2.), vec2(3., 4.)), 5.);
    LcBag other = bag; other.v[1].x = 9.;
    r = vec4(ps[0].x + ps[1].x, float(ps[0].n*ps[1].n), bag.v[1].x + bag.k, other.v[1].x + other.v[0].y);
""", (4, 6, 8, 11), "struct LcP { float x; int n; };\nstruct LcBag { vec2 v[2]; float k; };")
row("aggregates", "array: `out` parameter and return value", "6.1.1", """
    float v[3]; lc_fill(v, 2.);
    float p[2] = lc_pair(3.);
    r = vec4(v[0] + v[1], v[2], p[0]*10. + p[1], lc_pair(1.)[1]);
""", (6, 6, 36, 2), "void lc_fill(out float v[3], float s) { for (int i = 0; i < 3; i++) v[i] = s*float(i + 1); }\n"
                    "float[2] lc_pair(float x) { return float[2](x, x*2.); }")
row("aggregates", "array: constant globals, sized and unsized", "4.3.2", """
    r = vec4(LC_W[0] + LC_W[1], LC_U[1], LC_U.length(), LC_W.length());
""", (0.75, 2, 2, 3), "const float LC_W[3] = float[3](0.25, 0.5, 0.25);\nconst float LC_U[] = float[](1., 2.);")

# ---- structs (§4.1.8, §5.4.3, §5.9) -----------------------------------------------------------------------------------------------
row("aggregates", "struct: constructor with int -> float members", "5.4.3", """
    LcS s = LcS(1, vec2(2, 3), 4);
    r = vec4(s.a/2, s.b, s.c);
""", (0.5, 2, 3, 4), "struct LcS { float a; vec2 b; int c; };")
row("aggregates", "struct: constructor with an array member", "5.4.3", """
    LcHold h = LcHold(float[4](1., 2., 3., 4.), 5);
    r = vec4(h.w[0], h.w[3], h.n, h.w.length());
""", (1, 4, 5, 4))
row("aggregates", "struct: assignment copies, nested structs", "5.8", """
    LcOuter a = LcOuter(LcInner(vec2(1., 2.)), 3.);
    LcOuter b = a; b.i.p.x = 9.; b.k = 4.;
    r = vec4(a.i.p.x, a.k, b.i.p.x, b.k);
""", (1, 3, 9, 4), "struct LcInner { vec2 p; };\nstruct LcOuter { LcInner i; float k; };")
row("aggregates", "struct: `inout` parameter and return value", "6.1.1", """
    LcS s = LcS(1., vec2(0.), 4);
    LcS old = lc_bump(s);
    r = vec4(old.a, s.a, old.c, s.c);
""", (1, 2, 4, 5), "LcS lc_bump(inout LcS s) { LcS old = s; s.a += 1.; s.c++; return old; }")
row("aggregates", "struct: == and != compare the members", "5.9", """
    LcS x = LcS(1., vec2(2., 3.), 4), y = LcS(1., vec2(2., 3.), 4);
    r.xy = vec2(lc_b(x == y), lc_b(x != y));
    y.b.y = 5.;
    r.zw = vec2(lc_b(x == y), lc_b(x != y));
""", (1, 0, 0, 1))
row("aggregates", "struct: == with array and struct members", "5.9", """
    LcBag p = LcBag(vec2[2](vec2(1., 2.), vec2(3., 4.)), 5.); LcBag q = p;
    LcOuter a = LcOuter(LcInner(vec2(1., 2.)), 3.); LcOuter b = a;
    r.xy = vec2(lc_b(p == q), lc_b(a != b));
    q.v[1].y = 0.; b.i.p.x = 0.;
    r.zw = vec2(lc_b(p == q), lc_b(a != b));
""", (1, 0, 0, 1))

# ---- swizzle l-values (§5.5) ------------------------------------------------------------------------------------------------------
row("silent", "swizzle: v.wzyx = v, a.zyx = a, b.yx = b, c.yxwz = c.xyzw", "5.5", """
    vec4 v=vec4(1,2,3,4); v.wzyx = v;
    vec3 a=vec3(1,2,3); a.zyx = a;
    vec2 b=vec2(1,2); b.yx = b;
    vec4 c=vec4(1,2,3,4); c.yxwz = c.xyzw;
    r = vec4(v.x*10+v.y, a.x*10+a.z, b.x*10+b.y, c.x*10+c.w);
""", (43, 31, 21, 23))
row("vectors", "swizzle: v.xy = v.yx, v.yzw = v.xyz", "5.5", """
    vec4 v = vec4(1,2,3,4); v.xy = v.yx;
    vec4 u = vec4(1,2,3,4); u.yzw = u.xyz;
    r = vec4(v.x*10+v.y, u.y*100+u.z*10+u.w, u.x, v.z);
""", (21, 123, 1, 3))
row("vectors", "swizzle: w.xy += w.yx, u.zx *= u.xz", "5.5", """
    vec4 w = vec4(1,2,3,4); w.xy += w.yx;
    vec4 u = vec4(2,3,5,7); u.zx *= u.xz;
    vec4 t = vec4(2,3,5,7); t.zx *= t.xy;
    vec4 s = vec4(1,2,3,4); s.xy -= s.yx;
    r = vec4(w.x*10+w.y, u.z*100+u.x, t.z*10+t.x, s.x*10+s.y);
""", (33, 1010, 106, -9))
row("vectors", "swizzle: m[1].xy = m[1].yx, m[0] = m[1]", "5.5", """
    mat2 m = mat2(1,2,3,4); m[1].xy = m[1].yx;
    mat2 n = mat2(1,2,3,4); n[0] = n[1]; n[1].x = 9.;
    r = vec4(m[1].x*10+m[1].y, n[0].x*10+n[0].y, n[1].x, m[0].x);
""", (43, 34, 9, 1))
row("vectors", "swizzle: chained a = u.zw = value", "5.8", """
    vec4 u = vec4(1,2,3,4); vec2 a;
    a = u.zw = vec2(7., 8.);
    r = vec4(a, u.zw);
""", (7, 8, 7, 8))
row("vectors", "swizzle: rgba and stpq letters, v[k] with a variable k", "5.5", """
    vec4 v = vec4(1,2,3,4); v.bgr = v.rgb;
    v.ts = v.pq;
    int k = two;
    v[k] = 9.; float e = v[k - 1];
    r = vec4(v.x*10+v.y, v.z, v.w, e);
""", (41, 9, 4, 1))
row("vectors", "swizzle: the same forms on ivec and uvec", "5.5", """
    ivec4 v = ivec4(1,2,3,4); v.wzyx = v;
    ivec3 a = ivec3(1,2,3); a.zyx = a;
    uvec2 b = uvec2(1u,2u); b.yx = b;
    ivec4 w = ivec4(1,2,3,4); w.xy += w.yx; w.zw = w.wz;
    r = vec4(v.x*10+v.y, a.x*10+a.z, b.x*10u+b.y, w.x*1000+w.y*100+w.z*10+w.w);
""", (43, 31, 21, 3343))

# ---- constructors (§5.4.1-5.4.2) --------------------------------------------------------------------------------------------------
row("vectors", "constructor: scalar from bool, int, uint and a vector's first component", "5.4.1", """
    vec3 d = vec3(4., 5., 6.);
    float f = float(d.zyx); float g = float(d);
    int i = int(vec2(7.5, 1.)); uint u = uint(ivec2(9, 1));
    r = vec4(float(true) + float(7)*2. + float(3u)*16., f, g + float(ivec2(3, 4))*10., float(i) + float(u));
""", (63, 6, 34, 16))
row("vectors", "constructor: bool(2), bool(-0.5), bool of zeros", "5.4.1", """
    r = vec4(lc_b(bool(2)), lc_b(bool(-0.5)), lc_b(bool(0)), lc_b(bool(0.0)));
""", (1, 1, 0, 0))
row("vectors", "constructor: bvec from ivec and vec", "5.4.1", """
    bvec3 a = bvec3(ivec3(0, 2, -1)); bvec2 b = bvec2(vec2(0., 0.5));
    r = vec4(vec3(a), lc_b(b.y) + 2.*lc_b(b.x));
""", (0, 1, 1, 1))
row("vectors", "constructor: vectors from scalars and vectors, truncation", "5.4.2", """
    vec4 v4 = vec4(1,2,3,4);
    vec3 a = vec3(v4); vec2 b = vec2(v4);
    vec4 c = vec4(b, 5, a.z); vec4 d = vec4(1, vec2(2, 3), 4);
    r = vec4(a.z, b.y, c.z*10+c.w, d.y*10+d.z);
""", (3, 2, 53, 23))
row("vectors", "constructor: ivec(vec) truncates toward zero, uint(-1), int(0xFFFFFFFFu)", "5.4.1", """
    ivec4 t = ivec4(vec4(1.9, -1.9, 0.5, -0.5));
    uint u = uint(-1); int i = int(0xFFFFFFFFu);
    r = vec4(t.x, t.y, t.z + t.w, float(u >> 16) + float(i));
""", (1, -1, 0, 65534))
row("vectors", "constructor: matrices diagonal, from ints, from columns", "5.4.2", """
    mat2 a = mat2(2.); mat3 b = mat3(1,2,3,4,5,6,7,8,9); mat2 c = mat2(vec2(1,2), vec2(3,4));
    r = vec4(a[0][0]*1000.+a[0][1]*100.+a[1][0]*10.+a[1][1], b[2][1]*10.+b[1].z, c[1][0]*10.+c[0][1], b[0][0]);
""", (2002, 86, 32, 1))
row("vectors", "constructor: matrix from a larger and a smaller matrix, mat2(vec4)", "5.4.2", """
    mat3 b = mat3(1,2,3,4,5,6,7,8,9);
    mat2 s = mat2(b); mat3 g = mat3(mat2(1,2,3,4));
    mat2 d = mat2(vec4(1,2,3,4));
    r = vec4(s[1][0]*10.+s[1][1], g[1][0]*100.+g[1][2]*10.+g[2][2], d[1][0]*10.+d[0][1], g[2][0]);
""", (45, 301, 32, 0))

# ---- operators (§5.9) -------------------------------------------------------------------------------------------------------------
row("vectors", "operator: ++ and -- on scalars and components", "5.9", """
    int i = 5; int a = i++; int b = ++i;
    float f = 1.5; float c = f--; float d = --f;
    vec2 v = vec2(1., 2.); v.x++; --v.y; float e = v.y++;
    r = vec4(a*10+b, c + d, v.x*10.+v.y, e + float(i));
""", (57, 1, 22, 8))
row("vectors", "operator: ++ and -- on vectors, ivecs, uvecs and swizzles", "5.9", """
    vec4 v = vec4(1,2,3,4); ivec4 iv4 = ivec4(1,2,3,4);
    v++; iv4++;
    vec4 o = v--; --v;
    ivec2 iv = ivec2(1, -1); iv++; ivec2 io = iv++; ++iv;
    uvec2 uv = uvec2(0u, 5u); uv--;
    vec4 s = vec4(1,2,3,4); s.zx++;
    r = vec4(v.x + v.w*10. + s.x*100. + s.z*1000., o.y*10.+o.z, float(iv.x*10 + iv.y + io.x*100 + iv4.w*1000), float(uv.x >> 24) + float(uv.y));
""", (4230, 34, 5242, 259))
row("vectors", "operator: v *= m, m *= m, m*v, v*m", "5.9", """
    mat2 m = mat2(1,2,3,4); vec2 v = vec2(1., 1.);
    vec2 w = vec2(1., 2.); w *= m;
    mat2 n = m; n *= m;
    r = vec4((m*v).x*10.+(m*v).y, (v*m).x*10.+(v*m).y, w.x*100.+w.y, (n[0].x+n[1].x)*100.+n[0].y+n[1].y);
""", (46, 37, 511, 2232))
row("vectors", "operator: == and != on vectors, a swizzle, matrices and bvec", "5.9", """
    vec3 a = vec3(1,2,3); vec4 b = vec4(3,2,1,0);
    r = vec4(lc_b(a == b.zyx) + 2.*lc_b(a != b.zyx), lc_b(a != b.xyz) + 2.*lc_b(a == b.xyz),
             lc_b(mat2(1,2,3,4) == mat2(vec4(1,2,3,4))) + 2.*lc_b(mat2(1,2,3,4) != mat2(1,2,3,5)),
             lc_b(lessThan(a, vec3(2.)) == bvec3(true,false,false)) + 2.*lc_b(lessThan(a, vec3(2.)) != bvec3(true,false,false)) + 4.*lc_b(bvec2(true, false) != bvec2(true, true)));
""", (1, 1, 3, 5))
row("vectors", "operator: ivec & | ^ ~ against a scalar and a vector", "5.9", """
    ivec2 a = ivec2(12, -8); ivec2 b = ivec2(10, 3);
    r = vec4((a & b).x*100 + (a & 12).y, (a | b).y*100 + (a | 1).x, (a ^ b).x*100 + (a ^ -1).y, (~a).x*100 + (~a).y);
""", (808, -487, 607, -1293))
row("vectors", "operator: ivec << >> (arithmetic on negatives) and %", "5.9", """
    ivec2 a = ivec2(12, -8); ivec2 c = ivec2(13, 7);
    r = vec4((a << 2).x*100 + (a << ivec2(1, 2)).y, (a >> 1).y*100 + (a >> ivec2(2, 1)).x, (c % 5).x*10 + (c % 5).y, (c % ivec2(4, 3)).x*10 + (c % ivec2(4, 3)).y);
""", (4768, -397, 32, 11))
row("vectors", "operator: unary minus on uint, ^^, the sequence operator, ternaries", "5.9", """
    uint u = 1u; uint n = -u;
    bool t = true, f = false;
    int i = 0; int s = (i++, i++, i + 10);
    vec4 v = vec4(1,2,3,4); bool c = two > 1;
    vec2 p = c ? v.zw : vec2(9., 9.); vec2 q = c ? vec2(9., 8.) : v.xy;
    float m = c ? 1 : 2.5; float k = !c ? 1 : 2.5;
    r = vec4(float(n >> 16), lc_b(t ^^ f) + 2.*lc_b(t ^^ t) + 4.*lc_b(f ^^ f), float(s*10 + i), p.x*1000. + p.y*100. + q.y*10. + m + k);
""", (65535, 1, 122, 3483.5))
row("vectors", "operator: int / float mixing", "4.1.10", """
    vec2 h = vec2(1,2)/2; vec2 v = vec2(1., 2.); vec2 g = 2*v+1;
    float t = 1/3; float s = 1/2.;
    r = vec4(h.x + h.y*4., g.x*10.+g.y, t, s);
""", (4.5, 35, 0, 0.5))
row("vectors", "operator: int and uint wrap around", "4.1.3", """
    int big = 2147483647; big += two - 1;
    uint z = 0u; z -= uint(two) - 1u;
    int p = 65536*(65534 + two);
    r = vec4(float(big), float(z >> 16), float(p), float(3000000000u + 3000000000u));
""", (-2147483648.0, 65535, 0, 1705032704.0))

# ---- functions (§6.1) -------------------------------------------------------------------------------------------------------------
row("functions", "function: `in` parameters written locally, const in, out, inout", "6.1.1", """
    float x = 1.; vec2 v = vec2(2., 3.); LcT s = LcT(4., 0);
    float t = lc_in(x, v, s);
    float o; lc_out(o);
    float io = 2.; lc_inout(io);
    r = vec4(t, x + v.x*10. + s.a*100., o + lc_cin(o), io);
""", (20, 421, 15, 6), """struct LcT { float a; int c; };
float lc_in(float x, vec2 v, LcT s) { x += 1.; v.x = 9.; s.a = 9.; return x + v.x + s.a; }
float lc_cin(const in float x) { return x*2.; }
void lc_out(out float x) { x = 5.; }
void lc_inout(inout float x) { x *= 3.; }""")
row("functions", "function: an `out` parameter that reads a global before returning", "6.1.1", """
    lc_base = 1.;
    float o; lc_outg(o);
    r = vec4(o, lc_base, 0., 0.);
""", (6, 1, 0, 0), "float lc_base = 1.;\nvoid lc_outg(out float x) { x = 5.; x += lc_base; }")
row("functions", "function: a swizzle and a matrix column as `out` / `inout` arguments", "5.5", """
    vec4 v = vec4(1,2,3,4);
    lc_set(v.zw); lc_twice(v.yx);
    mat2 m = mat2(1.); lc_set(m[1]);
    vec4 w = vec4(1.5, 2.25, 0., 0.); vec2 frac_ = modf(w.xy, w.zw);
    r = vec4(v.x*10.+v.y, v.z*10.+v.w, m[1].x*10.+m[1].y + m[0].x*100., w.z*10. + w.w + frac_.x + frac_.y);
""", (24, 78, 178, 12.75), "void lc_set(out vec2 p) { p = vec2(7., 8.); }\nvoid lc_twice(inout vec2 p) { p *= 2.; }")
row("functions", "function: arguments and constructor arguments are evaluated left to right", "6.1.1", """
    lc_count = 0;
    float p = lc_pack(lc_next(), lc_next(), lc_next());
    vec3 v = vec3(lc_next(), lc_next(), lc_next());
    r = vec4(p, v.x*100.+v.y*10.+v.z, float(lc_count), 0.);
""", (123, 456, 6, 0), "int lc_count = 0;\nfloat lc_next() { lc_count++; return float(lc_count); }\nfloat lc_pack(float a, float b, float c) { return a*100. + b*10. + c; }")
row("functions", "function: && and || do not evaluate their right side", "5.9", """
    lc_count = 0;
    bool a = false && (lc_next() > 0.); bool b = true || (lc_next() > 0.);
    bool c = true && (lc_next() > 0.); bool d = false || (lc_next() > 5.);
    r = vec4(lc_b(a), lc_b(b), lc_b(c) + 2.*lc_b(d), float(lc_count));
""", (0, 1, 1, 2))
row("functions", "function: overloads on int, float and vec2; int -> float where only float exists", "6.1", """
    r = vec4(lc_ov(1), lc_ov(1.), lc_ov(vec2(1.)), lc_only(3));
""", (1, 2, 3, 1.5), "float lc_ov(int x) { return 1.; }\nfloat lc_ov(float x) { return 2.; }\nfloat lc_ov(vec2 x) { return 3.; }\nfloat lc_only(float x) { return x/2.; }")
row("functions", "function: prototypes, f(void), globals changed through nested calls", "6.1", """
    lc_state = 0.5; lc_outer();
    r = vec4(lc_early(3.), lc_none(), lc_state, 0.);
""", (7, 4, 5, 0), """float lc_later(float x);
float lc_early(float x) { return lc_later(x) + 1.; }
float lc_later(float x) { return x*2.; }
float lc_none(void) { return 4.; }
float lc_state = 0.;
void lc_inner() { lc_state += 1.; }
void lc_outer() { lc_inner(); lc_inner(); lc_state *= 2.; }""")

# ---- statements (§6.2-6.4) --------------------------------------------------------------------------------------------------------
row("functions", "statement: switch with fall-through, braces and default; do/while/continue; for(;;) break; two declarators and steps", "6.2", """
    int acc = 0;
    for (int k = 0; k < 5; k++) {
        switch (k) {
            case 0: acc += 1;
            case 1: acc += 10; break;
            case 2: { acc += 100; break; }
            case 3:
            default: acc += 1000;
        }
    }
    int i = 0, s = 0;
    do { i++; if (i == 2) continue; s += i; } while (i < 4);
    int n = 0;
    for (;;) { n++; if (n >= 3) break; }
    int t = 0;
    for (int a = 0, b = 10; a < b; a++, b--) t += b - a;
    r = vec4(acc, s, n, t);
""", (2121, 8, 3, 30))
row("functions", "statement: a nested loop that reuses the counter's name, a float counter", "6.3", """
    int s = 0;
    for (int i = 0; i < 3; i++) { for (int i = 0; i < 2; i++) s += 1; s += 10; }
    float f = 0.;
    for (float x = 0.; x < 1.; x += 0.25) f += x;
    r = vec4(s, f, 0., 0.);
""", (36, 1.5, 0, 0))
row("functions", "statement: early return from main", "6.4", """
    r = vec4(9.); fragColor = vec4(1., 2., 3., 4.);
    if (two == 2) return;
    fragColor = vec4(5.);
""", (1, 2, 3, 4))
row("functions", "statement: discard in main, nothing after it takes effect", "6.4", """
    r = vec4(5.); fragColor = r;
    if (two == 2) discard;
    r = vec4(6.);
""", (0, 0, 0, 0))
row("functions", "statement: discard inside a function", "6.4", """
    r = vec4(3.); r.x = lc_gone(float(two)); r.y = 7.;
""", (0, 0, 0, 0), "float lc_gone(float x) { if (x > 0.) discard; return 1.; }")

# ---- qualifiers and scope (§4.2, §4.3) --------------------------------------------------------------------------------------------
row("functions", "scope: chains of const as array bounds, global and local", "4.3.2", """
    const int n = LC_B; const int m = n + 1;
    float loc[m];
    lc_big[5] = 2.; loc[3] = 3.;
    r = vec4(lc_big.length(), loc.length(), lc_big[5], loc[3]);
""", (6, 4, 2, 3), "const int LC_A = 2;\nconst int LC_B = LC_A + 1;\nconst int LC_C = LC_B*2;\nfloat lc_big[LC_C];")
row("functions", "scope: a local const with a non-constant initialiser", "4.3.2", """
    const float c = float(two)*1.5; const vec2 v = vec2(c, c + 1.);
    r = vec4(c, v, 0.);
""", (3, 3, 4, 0))
row("functions", "scope: locals and parameters named like built-in functions, uniforms and varyings", "4.2", """
    float max = 2.; float mix = 3.; vec2 gluv = vec2(5., 6.);
    { float iFrame = 7.; r.w = iFrame; }
    r.xyz = vec3(lc_shadow(1., 2., vec2(3., 4.)), max*mix, gluv.y);
""", (7, 6, 6, 7), "float lc_shadow(float sin, float iTime, vec2 stuv) { float length = sin + iTime; return length + stuv.y; }")
row("functions", "scope: C++ keywords as identifiers", "3.6", """
    float new = 1.; float delete = 2.; float operator = 4.; float private = 8.; float try = 16.; float and = 32.; float final = 64.; float nullptr = 128.;
    r = vec4(new + delete + operator + private + try + and + final + nullptr, lc_kw(3., 1.), 0., 0.);
""", (255, 2, 0, 0), "float lc_kw(float virtual, float explicit) { float mutable = virtual - explicit; return mutable; }")

# ---- the text (§3) ----------------------------------------------------------------------------------------------------------------
# A probe of its own: directives and global-scope text that cannot sit inside another probe. The row order fixes its lines.
TEXT_HEAD = """#version 330
precision highp float;
precision mediump int;
#define LC_SQ(x) ((x)*(x))
#define LC_TWO \\
    2.0
#define LC_ADD(a, b) \\
    ((a) + \\
     (b))
#ifdef LC_TWO
#define LC_PICK 1.0
#else
#define LC_PICK 2.0
#endif
#ifdef LC_NOT_DEFINED
#define LC_OTHER 1.0
#else
#define LC_OTHER 2.0
#endif
highp float lc_p(mediump float x, lowp vec2 v) { highp float y = x + v.y; return y; }
"""
row("text", "text: #version, precision statements and qualifiers", "4.5", """
    mediump vec2 v = vec2(0., 2.); lowp int i = 3;
    r = vec4(lc_p(1., v), i, 0., 0.);
""", (3, 3, 0, 0))
row("text", "text: literals .5 5. 1e1 1.f 3.0lf, hex with u, octal, 3000000000u", "4.1.3", """
    r = vec4(.5 + 5. + 1e1 + 1.f, 3.0lf, float(0x1Fu) + float(010) + float(0xFF), float(3000000000u >> 8));
""", (16.5, 3, 294, 11718750))
row("text", "text: function-like macros, #ifdef / #else, a backslash-newline continuation", "3.3", """
    r = vec4(LC_SQ(1. + 2.), LC_TWO, LC_ADD(1., LC_TWO), LC_PICK*10. + LC_OTHER);
""", (9, 2, 3, 12))
LINE_ROW = "text: __LINE__ is the line of the fragment's text"       # its expectation is counted from the probe's text (probe_glsl)
row("text", LINE_ROW, "3.3", """
    r.x = float(__LINE__);
#define LC_INSIDE \\
    4.0
    r.y = float(__LINE__); r.z = LC_INSIDE;
#undef LC_INSIDE
""", (0, 0, 4, 0))

# "silent": the two rows that compiled and drew wrong numbers before these tables existed, in a probe that holds nothing else, so that
# it still builds against a header and a translator without the other rows' constructs and shows those numbers
PROBES = ("silent", "aggregates", "vectors", "functions", "text")
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
HELPERS = "uniform int group;\nuniform int two;\nfloat lc_b(bool b) { return b ? 1.0 : 0.0; }\n"
SIZE = (4, 4)


def rows_of(probe: str) -> list[Row]:
    return [r for r in ROWS if r.probe == probe]


def group_of(r: Row) -> int:
    return 1 + rows_of(r.probe).index(r)


def probe_glsl(probe: str) -> str:
    helpers = list(dict.fromkeys(r.helpers for r in rows_of(probe) if r.helpers))
    lines = [TEXT_HEAD if probe == "text" else "", HELPERS, *helpers, "void main() {", "    vec4 r = vec4(0.0);", "    switch (group) {"]
    for index, r in enumerate(rows_of(probe), 1):
        lines.append(f"        case {index}: {{      // {r.name} (§{r.section})\n    {r.body}\n        break; }}")
    lines += ["        default: r = vec4(-1.0); break;", "    }", "    fragColor = r;", "}"]
    return "\n".join(lines) + "\n"


def expected(r: Row) -> np.ndarray:
    want = np.array(r.want, F)
    if r.name == LINE_ROW:                    # §3.3: one more than the number of newlines before it
        text = probe_glsl(r.probe)
        first = text.index("float(__LINE__)")
        want[0] = 1 + text[:first].count("\n")
        want[1] = 1 + text[:text.index("float(__LINE__)", first + 1)].count("\n")
    return want


def evaluate(probe: str, render) -> dict:
    """`render(group)` -> (4, 4, 4) float32; {row name: that array}"""
    return {r.name: np.asarray(render(group_of(r)), F) for r in rows_of(probe)}


def check(probe: str, results: dict) -> None:
    """every pixel of every row equals the row's expectation; the message names each failing row and its section"""
    wrong = []
    for r in rows_of(probe):
        got, want = results[r.name], expected(r)
        assert got.shape == (SIZE[1], SIZE[0], 4), (r.name, got.shape)
        if not (got == want).all():
            wrong.append(f"{r.name} (GLSL 3.30 §{r.section}): want {want.tolist()}, got {got[0, 0].tolist()}"
                         + ("" if (got == got[0, 0]).all() else " (and other values at other pixels)"))
    assert not wrong, f"{probe}: {len(wrong)} of {len(rows_of(probe))} rows are wrong\n" + "\n".join(wrong)


def check_same(probe: str, results: dict, others: dict, what: str) -> None:
    assert set(results) == set(others) == {r.name for r in rows_of(probe)}
    wrong = [name for name in results if not np.array_equal(results[name].view(np.uint32), others[name].view(np.uint32))]
    assert not wrong, f"{probe}: {what}: the bits differ in {wrong}"


# ---- valid GLSL the translator refuses by name ------------------------------------------------------------------------------------
REFUSALS = [
    ("a keyword rename meeting its own result", "3.6", "void main() { float new=1.; float new_=2.; fragColor = vec4(new + new_); }", "'new' and 'new_'"),
    ("&& next to ^^ without parentheses", "5.9", "void main() { bool a = true, b = false, c = true; fragColor = vec4(float(a && b ^^ c)); }", "`&&` next to `^^`"),
    ("an unsized array initialised from something other than a constructor", "4.1.9",
     "void main() { float a[2] = float[2](1., 2.); float b[] = a; fragColor = vec4(b[0]); }", "array 'b' is declared without a size"),
    ("a non-square matrix", "4.1.6", "void main() { mat2x3 m = mat2x3(1.); fragColor = vec4(m[0], 1.); }", "type mat2x3"),
    ("a sampler other than sampler2D", "4.1.7", "uniform sampler3D volume;\nvoid main() { fragColor = texture(volume, vec3(0.)); }", "type sampler3D"),
]

# ---- whole fragments for the entry points of a code object -------------------------------------------------------------------------
SEEN = "float seen = 1.0;\nvoid main(){ seen += 1.0; fragColor = vec4(seen/4.0); }\n"
CHECKER = ("void main() {\n    ivec2 at = ivec2(gl_FragCoord.xy);\n    fragColor = vec4(0.25, 0.5, 0.75, 1.0);\n"
           "    if (((at.x + at.y) & 1) == 1) discard;\n}\n")
KEPT = (0.25, 0.5, 0.75, 1.0)                 # what the checkerboard writes where x + y is even
# … and both in one fragment with a tap of a sampler that adds nothing (0.0*texel): translated with the LDS tile forced for `tex`, its
# code object runs the fragment once more per block to find the tile, and exports the quad-layout twin sfx_jit_render_quads. Where a
# sample is kept it holds KEPT*(seen/2) = KEPT
TAPPED = ("float seen = 1.0;\nvoid main() {\n    ivec2 at = ivec2(gl_FragCoord.xy);\n    seen += 1.0;\n"
          "    fragColor = vec4(0.25, 0.5, 0.75, 1.0)*(seen/2.0) + 0.0*texture(tex, astuv);\n    if (((at.x + at.y) & 1) == 1) discard;\n}\n")
PER_INVOCATION = {"seen": SEEN, "checker": CHECKER, "tapped": TAPPED}
