"""
The vector, matrix and integer built-ins of csrc/jit_runtime.hpp value by value, on the CPU: the probes of tests/vector_cases.py built
for the x86 host (tests/jit_host.py) against the float32 / int32 restatements (bit for bit), the scalar forms (component by component),
the float64 witnesses (derived bounds) and the inverse property. tests/test_gpu_vector.py holds the gfx950 build to the same bits.
"""
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import glsl2hip as G
from tests import math_cases as M
from tests import vector_cases as V
from tests.jit_host import HostFragment

ROOT = Path(__file__).resolve().parent.parent
CACHE = ROOT/"build"/"jit"
F = np.float32
_evaluations: dict = {}


def host_evaluation(fragment: str):
    """the fragment's probe on the host over every input of its rows: ({row: results}, {set: echo}); once per session"""
    if fragment not in _evaluations:
        host = HostFragment(G.translate(V.probe_glsl(fragment), V.PROBE_UNIFORMS), CACHE)
        host.set_uniforms(O.default_uniforms(*V.rows_of(fragment)[0].size))

        def render(group, column, four, size):
            host.set("group", group)
            host.set("column", column)
            for name, texels in zip(("opA", "opB", "opC", "opD"), four):
                assert host.bind(name, texels, "nearest", False, False)
            return host.render_float(*size)
        _evaluations[fragment] = V.evaluate(fragment, render)
    return _evaluations[fragment]


def test_the_inputs_are_whole_deterministic_and_cannot_trap():
    data = V.inputs()
    V.assert_clean(data)
    for name, (X, everyday) in data.items():
        assert X.dtype == F and X.shape[1] == 16 and len(X) % (16 if name == "swizzle" else V.POINTS) == 0 and len(everyday) == len(X), name
        assert len(X) <= 8*V.POINTS, name
    X, everyday = data["vec"]
    for slot in range(16):                                         # every special, bit for bit, in every slot
        assert set(M.bits(M.SPECIALS).tolist()) <= set(M.bits(X[:, slot]).tolist()), slot
    assert (np.abs(np.delete(X[everyday], 12, 1)) <= 4).all() and (np.abs(X[everyday, 12]) <= 2048).all() and everyday.sum() > 30000      # slot 12: refract's eta
    for n in (2, 3, 4):                                            # length: a zero vector, subnormals, overflow and underflow of the sum of squares
        a = X[:, :n].astype(np.float64)
        with np.errstate(over="ignore"):
            squares = (a.astype(F)**2).sum(1, dtype=F)
        assert ((a == 0).all(1)).sum() >= 200 and (np.isinf(squares) & np.isfinite(a).all(1)).sum() >= 200
        assert ((squares == 0) & (a != 0).any(1)).sum() >= 200 and ((np.abs(a) < M.FLT_MIN).all(1) & (a != 0).any(1)).sum() >= 200
        # refract: both sides of k = 0, and its float neighbours
        with np.errstate(all="ignore"):
            _, k = V.ref_refract([X[:, j] for j in range(n)], [X[:, 4 + j] for j in range(n)], X[:, 12])
        ordinary = np.isfinite(k) & (np.abs(X[:, :8]) <= 4).all(1)
        assert (k[ordinary] < 0).sum() > 1000 and (k[ordinary] >= 0).sum() > 1000 and (np.abs(k[ordinary]) <= 2.0**-20).sum() > 200, n
        assert (k[ordinary] == 0).sum() > 10, n
    for n in (2, 3, 4):
        X, conditioned = data[f"mat{n}"]
        m = X[:, V.MATRIX_SLOTS[n][0]].astype(np.float64).reshape(-1, n, n)
        assert conditioned.sum() > 8000 and np.linalg.cond(m[conditioned]).max() <= 100
        flat = m.reshape(len(m), -1)
        assert (flat == np.eye(n).reshape(-1)).all(1).sum() >= 8
        assert (np.abs(np.linalg.det(m[np.isfinite(flat).all(1)])) < 1e-12).sum() >= 100            # singular
        for slot in range(n*n):
            assert set(M.bits(M.SPECIALS).tolist()) <= set(M.bits(flat[:, slot].astype(F)).tolist()), (n, slot)
    W = V.floats_to_words(data["int"][0])
    pairs = set(zip(W[:, 0].tolist(), W[:, 4].tolist()))
    assert all((int(a), int(b)) in pairs for a in V.INT_SPECIALS for b in V.INT_SPECIALS)
    assert np.array_equal(V.words_to_floats(W), data["int"][0])
    assert set(range(32)) <= set(V.floats_to_words(data["shift"][0])[:, 4].tolist())
    again = {name: X.copy() for name, (X, _) in data.items()}
    V.reset()
    assert all(np.array_equal(M.bits(V.inputs()[name][0]), M.bits(again[name])) for name in again)


def test_the_table_walks_the_header():
    names = " ".join(V.BY_NAME)
    for wanted in V.MAP1 + ["dot", "length", "distance", "normalize", "cross", "reflect", "faceforward", "refract", "lessThan", "notEqual(bvec",
                            "any, all", "not(", "isnan(vec3", "isinf(vec2", "mix(vec4, vec4, bvec4)", "modf(vec3", "inverse", "determinant", "outerProduct",
                            "transpose", "matrixCompMult", "uvec3: min(a, scalar)", "ivec4: abs(a)", "uint: clamp(a, b, c)", "ivec2: a % b", "uvec4: a >>= scalar",
                            "vec4.wzyx", "ivec4.zx = t", "v.xy = v.yx", "floatBitsToUint(vec3)"]:
        assert wanted in names, wanted
    # … and the header's own lists: every function a SF_RT_MAP* macro maps over vec2/3/4, every relation, every prelude function
    header = (G.CSRC/"jit_runtime.hpp").read_text()
    mapped = {macro: set(re.findall(rf"(?<!define ){macro}\((\w+)\)", header)) for macro in ("SF_RT_MAP1", "SF_RT_MAP2", "SF_RT_MAP2S")}
    assert mapped["SF_RT_MAP1"] - {"dFdx", "dFdy", "fwidth"} == set(V.MAP1), mapped["SF_RT_MAP1"] ^ set(V.MAP1)       # derivatives: out of scope
    for n in (2, 3, 4):
        for name in V.MAP1:
            assert f"{name}(vec{n})" in V.BY_NAME, name
        for name in mapped["SF_RT_MAP2"]:
            assert len(mapped["SF_RT_MAP2"]) == 6 and f"{name}(vec{n}, vec{n})" in V.BY_NAME, name
        for name in mapped["SF_RT_MAP2S"]:
            assert len(mapped["SF_RT_MAP2S"]) == 3 and f"{name}(vec{n}, float)" in V.BY_NAME, name
        body = header[header.index("#define SF_RT_MAP3(V, N)"):header.index("SF_RT_MAP3(vec2, 2)")]
        for name in set(re.findall(r"SF_HD \w+ (\w+)\(", body)):
            assert any(row.startswith(f"{name}(vec{n}") for row in V.BY_NAME), (name, n)
        for name in re.findall(r"(?<!define )SF_RT_REL\((\w+),", header):
            assert all(row in V.BY_NAME for row in (f"{name}(vec{n})", f"ivec{n}: {name}(a, b)", f"uvec{n}: {name}(a, b)")), (name, n)
    prelude = header[header.index("// ---- prelude: include/shaderflow.glsl"):header.index("// ---- prelude: include/camera.glsl")]
    bodies = " ".join(row.body for row in V.rows_of("prelude"))
    functions = set(re.findall(r"^SF_HD \w+ (\w+)\(", prelude, re.M)) | set(re.findall(r"^#define (\w+)\(", prelude, re.M))
    sampling = {"gtexture", "stexture", "astexture", "_sdLine"}          # the texture functions are out of scope; _sdLine is sdLine's helper
    assert len(functions) > 60 and not [name for name in functions - sampling if not re.search(rf"\b{name}\(", bodies)], \
        [name for name in functions - sampling if not re.search(rf"\b{name}\(", bodies)]
    assert len([r for r in V.ROWS if r.fragment == "swizzle" and r.name.startswith("vec4.") and len(r.name) == 9 and "=" not in r.name]) >= 256
    for row in V.ROWS:
        assert row.ref is not None or row.like is not None or row.within is not None or "device = host" in row.note, row.name


@pytest.mark.parametrize("form", list(V.ADDED_FORMS))
def test_added_form_compiles(form):
    """each form this table added to jit_runtime.hpp, in a fragment of its own: a missing overload fails here under the form's name"""
    text = "void main() { " + V.ADDED_FORMS[form] + " }\n"
    unit = CACHE/f"form_{list(V.ADDED_FORMS).index(form)}_{os.getpid()}.hip"
    CACHE.mkdir(parents=True, exist_ok=True)
    unit.write_text(G.translate(text, []).cpp)
    done = subprocess.run([G.HIPCC, *G.FLAGS, "--offload-host-only", "-DSF_JIT_HOST", "-fsyntax-only", f"-I{G.CSRC}", str(unit)], capture_output=True, text=True, timeout=300)
    unit.unlink()
    assert done.returncode == 0, f"{form} does not compile:\n{done.stderr[-1500:]}"


@pytest.mark.parametrize("fragment", V.FRAGMENTS)
def test_operands_come_back_bit_for_bit(fragment):
    V.check_echo(host_evaluation(fragment)[1])


@pytest.mark.parametrize("fragment", V.FRAGMENTS)
def test_rows_equal_their_restatements_bit_for_bit(fragment):
    V.check_exact(fragment, host_evaluation(fragment)[0])


@pytest.mark.parametrize("fragment", ("geometric", "matrix"))
def test_float64_witnesses_keep_their_derived_bounds(fragment):
    V.check_witness(fragment, host_evaluation(fragment)[0])


def test_inverse_times_the_matrix_is_the_identity():
    results = host_evaluation("matrix")[0]
    V.check_inverse(results)
    for n in (2, 3, 4):                                            # the bound comes from the numpy restatement alone, and is recorded next to it
        row = V.BY_NAME[f"mat{n}: inverse"]
        X, conditioned = V.inputs()[row.inputs]
        own = float(V.inverse_residual(X, np.asarray(row.ref(X), F), n)[conditioned].max())
        bound, measured = V.INVERSE_RESIDUAL[n]
        assert own == pytest.approx(measured, rel=1e-3) and bound/2 < measured <= bound, (n, own, bound, measured)
