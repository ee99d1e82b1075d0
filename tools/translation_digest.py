#!/usr/bin/env python3
"""One line per fragment of a fixed corpus: what glsl2hip.translate makes of it (sha256 of the C++ text, the bindings, the tiled
sampler) or REFUSED and the message. No GPU, no hipcc. A refactor of the translator must leave this output as it is; the time of the
translate loop alone goes to stderr.
usage: python tools/translation_digest.py > digest.txt"""
import hashlib
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
os.environ.pop("SHADERFLOW_JIT_TILE", None)
from examples.scenes import Bloom, PianoRoll                                      # noqa: E402
from shaderflow_amd.glsl2hip import TranslationError, translate                   # noqa: E402
from tests import language_cases as L, math_cases as M, texture_cases as T, vector_cases as V      # noqa: E402

BACKGROUND = [("sampler2D", "background")]
PIANO = ("Keys", "Chan", "Roll", "Tempo")                                         # as tests/test_piano_schedule.py assembles the fragment
PIANO_VARIABLES = [("sampler2D", f"iPiano{name}0x0") for name in PIANO] + [
    ("int", "iPianoGlobalMin"), ("int", "iPianoGlobalMax"), ("vec2", "iPianoDynamic"), ("float", "iPianoRollTime"),
    ("float", "iPianoExtra"), ("float", "iPianoHeight"), ("int", "iPianoLimit"), ("float", "iPianoBlackRatio")]
EDGES = [       # the seams between text and tokens: every one translates or is refused by name
    "uniform vec2 a = vec2(1, 2), b; uniform float /* gain */ g = 2.0*3.0;\nvoid main() { fragColor = vec4(a, b.x, g); }",
    "const int N = 3;\nuniform float w[N];\nuniform vec2[2] p = vec2[2](vec2(1), vec2(2, 3));\nuniform mat2 m = mat2(2.0);\nvoid main() { fragColor = vec4(w[0], p[1], m[1].y); }",
    "uniform float w[2][2];\nvoid main() { fragColor = vec4(w[0][0]); }",
    "uniform float g = sqrt(2.0);\nvoid main() { fragColor = vec4(g); }",
    "in vec2 stuv, extra[2];\nout vec4 fragColor;\nflat in int which;\nvoid main() { fragColor = vec4(extra[1], which, 1); }",
    "float table[3] = float[3](1., 2., 3.);\nstruct S { float a; vec2 b; } ;\nS s = S(1., vec2(2.));\nvoid main() { fragColor = vec4(table[1], s.b, s.a); }",
    "#define TAP(o) texture(background, astuv + o)\nvoid main() { fragColor = TAP(0.)+TAP(.1)+TAP(.2)+TAP(.3)+TAP(.4)+TAP(.5)+TAP(.6)+TAP(.7)+TAP(.8); }",
    "vec4 one(sampler2D t, vec2 uv) { return texture(t, uv); }\nvoid main() { vec4 s = vec4(0); for (int k = 0; k < 9; k++) s += one(background, stuv + 0.01*k); fragColor = s; }",
    "void f(out float a);\nvoid f(float a, inout vec2 b) { b *= a; }\nvoid f(out float a) { a = 1.; }\nvoid main() { vec4 v = vec4(1); f(v.x); f(2., v.zw); fragColor = v; }",
    "#define new 2.0\n#define K(x) \\\n   (x*new)\nvoid main() {\n#ifdef K\n fragColor = vec4(K(1.5));\n#endif\n}",
    "const int A = 2, B = A*3;\nconst uint C = uint(B);\nconst float D = float(A)/2.;\nconst bool E = true;\nfloat arr[B];\nvoid main() { fragColor = vec4(arr.length(), C, D, E); }",
    "void main() { bool a = true, b = false; fragColor = vec4((a && b) ^^ a, a ^^ b || a, 0, 1); }",
    "float x = 1.0\nvoid main() {}",
    "layout(std140) uniform Block { float a; };\nvoid main() {}",
    "#define REP(n) for (int i = 0; i < n; i++)\nvoid main() { fragColor = texture(background, stuv); }",
    "#define REAL float\nREAL f(out vec2 a) { a = vec2(1); return 1.; }\nvoid main() { vec4 v = vec4(0); f(v.xy); fragColor = v; }",
    "in vec2 extra[2], mine;\nflat in int ids[2], one;\nin vec2 more, pair[2], stuv;\nvoid main() { fragColor = vec4(extra[1], mine); }",
    "uniform uint[2] new;\nout mat2 b[] = mat2[](mat2(1,2,3,4), mat2(1)), c;\nvoid main() { fragColor = vec4(new[0]); }",
    "void main() { vec4 s = vec4(0); for (int i = 0; i < 2; i++) if (i > 0) discard; s += texture(background, stuv); fragColor = s; }",
]

corpus = [(f"language/{p}", L.probe_glsl(p), []) for p in L.PROBES]
corpus += [(f"language/{name}", text, [("sampler2D", "tex")]) for name, text in L.PER_INVOCATION.items()]
corpus += [(f"language/refusal/{k}", refusal[2], []) for k, refusal in enumerate(L.REFUSALS)]
corpus += [(f"vector/{f}", V.probe_glsl(f), V.PROBE_UNIFORMS) for f in V.FRAGMENTS]
corpus += [("math", M.probe_glsl(), M.PROBE_UNIFORMS)]
corpus += [(f"texture/{name}", text, T.PROBE_UNIFORMS) for name, text in (
    ("explicit", T.probe_glsl(T.EXPLICIT_FORMS)), ("proj", T.probe_glsl(T.PROJ_FORMS)), ("blur", T.BLUR_GLSL), ("bias", T.BIAS_GLSL))]
for path in sorted((ROOT/"tests"/"golden"/"jit").glob("*.glsl")):
    corpus += [(f"golden/{path.stem}", path.read_text(), []), (f"golden/{path.stem}+background", path.read_text(), BACKGROUND)]
corpus += [("bloom", Bloom.FRAGMENT, BACKGROUND)]
corpus += [("pianoroll", "".join(f"#define iPiano{name} iPiano{name}0x0\n" for name in PIANO) + PianoRoll.FRAGMENT, PIANO_VARIABLES)]
corpus += [(f"edge/{k}", text, BACKGROUND) for k, text in enumerate(EDGES)]

results = []
started = time.perf_counter()
for name, text, uniforms in corpus:
    try:
        results.append((name, translate(text, uniforms)))
    except TranslationError as error:
        results.append((name, error))
print(f"{len(corpus)} translations in {time.perf_counter() - started:.4f} s", file=sys.stderr)
for name, result in results:
    if isinstance(result, TranslationError):
        print(name, "REFUSED", result)
    else:
        bindings = [(b.name, b.type, b.slot, b.count, b.integer, b.default, b.array) for b in result.bindings]
        print(name, hashlib.sha256(result.cpp.encode()).hexdigest(), bindings, result.tiled_sampler)
