"""
The GLSL built-ins of csrc/jit_runtime.hpp value by value, on the CPU: the probe of tests/math_cases.py built for the x86 host
(tests/jit_host.py) against the oracle's restatement (bit for bit), the numpy float32 restatements (bit for bit), float64 numpy
(bounds) and the properties that hold on every finite input. tests/test_gpu_math.py holds the gfx950 build to the same bits.
"""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import glsl2hip as G
from tests import math_cases as M
from tests.jit_host import HostFragment

ROOT = Path(__file__).resolve().parent.parent
CACHE = ROOT/"build"/"jit"
F = np.float32


def host_evaluation():
    """the probe on the host over every input: ({case: results}, {arity: echo})"""
    host = HostFragment(G.translate(M.probe_glsl(), M.PROBE_UNIFORMS), CACHE)
    host.set_uniforms(O.default_uniforms(M.WIDTH, M.HEIGHT))

    def render(group, texels):
        host.set("group", group)
        assert host.bind("operands", texels, "nearest", False, False)
        return host.render_float(M.WIDTH, M.HEIGHT)
    return M.evaluate(render)


@pytest.fixture(scope="module")
def evaluation():
    return host_evaluation()


@pytest.fixture(scope="module")
def results(evaluation):
    return evaluation[0]


def test_the_table_has_every_scalar_built_in_and_the_inputs_every_special():
    names = {c.name.split(".")[0].split("(")[0] for c in M.CASES}
    wanted = ("radians degrees sin cos tan atan atan2 asin acos exp log exp2 log2 pow sqrt inversesqrt sinh cosh tanh abs sign floor ceil trunc round "
              "roundEven fract mod min max clamp mix step smoothstep fma modf isnan isinf int uint floatBitsToInt intBitsToFloat").split()
    assert set(wanted) <= names, set(wanted) - names
    header = (G.CSRC/"jit_runtime.hpp").read_text()
    for name in wanted:                                            # … and the header defines each as a scalar form
        function = {"atan2": "atan", "int": "to_int", "uint": "to_uint"}.get(name, name)
        assert re.search(rf"SF_HD (float|bool|int|uint) {function}\(", header), name
    assert sorted(O.MATH_FN) == M.ORACLE_FUNCTIONS and len(M.ORACLE_FUNCTIONS) == 13
    data = M.inputs()
    for arity in (1, 2, 3):
        assert data[arity].shape[0] % M.POINTS == 0 and data[arity].shape[1] == arity and data[arity].dtype == F
    for arity, specials in ((1, M.SPECIALS), (2, M.SPECIALS), (3, M.SPECIALS)):
        for slot in range(arity):                                  # every special, bit for bit, in every operand slot
            assert set(M.bits(specials).tolist()) <= set(M.bits(data[arity][:, slot]).tolist()), (arity, slot)
    again = dict(data)
    M._cache.clear()
    assert all(np.array_equal(M.bits(M.inputs()[k]), M.bits(again[k])) for k in again)         # generated, deterministic


def test_operands_come_back_bit_for_bit(evaluation):
    M.check_echo(evaluation[1])


def test_host_build_equals_the_oracle_bit_for_bit(results):
    M.check_oracle(results)


def test_exact_built_ins_equal_their_float32_restatements(results):
    M.check_exact(results)


def test_approximate_built_ins_keep_their_bounds(results):
    M.check_approx(results)
    measured = M.measure(results)
    for case in M.CASES:                                           # the table's record is what the host build gives on these inputs
        if case.kind == "approx":
            assert measured[case.name] == pytest.approx(case.measured, abs=0.006), case.name
            assert case.measured <= case.bound


def test_sin_and_cos_next_to_their_zeros(results):
    M.check_circular(results)


def test_the_reach_is_the_last_binade_sfmaths_reduction_keeps_its_bound_on():
    """Why SINCOS_REACH is 2^20: the sequences of sfmath (here through the oracle, the same bits) over a dense sample of the binade
    below it keep 4 ulp away from the zeros and 2.5e-7 everywhere; in the upper half of the binade above it they no longer do
    (measured: 1.65 ulp / 9.8e-8 in [2^19, 2^20), 5.41 ulp / 3.2e-7 in [1.5*2^20, 2^21), 3e-4 at 2^24, 0.03 at 1.5*2^24)"""
    rng = np.random.default_rng(1)
    worst = {}
    for lo, hi in ((2.0**19, 2.0**20), (1.5*2.0**20, 2.0**21)):
        x = rng.uniform(lo, hi, 6000).astype(F)*rng.choice([-1, 1], 6000).astype(F)
        want = np.sin(x.astype(np.float64))
        got = O.math("sin", x)
        away = ~M.circular_classes(x)[0]
        worst[lo] = (float(M.ulp_error(got, want)[away].max()), float(np.abs(got - want).max()))
    print(worst)
    assert worst[2.0**19][0] <= 4 and worst[2.0**19][1] <= M.ABSOLUTE_BOUND
    assert worst[1.5*2.0**20][0] > 4 and worst[1.5*2.0**20][1] > M.ABSOLUTE_BOUND
    assert float(M.SINCOS_REACH) == 2.0**20 and "SINCOS_REACH = 1048576.0f" in (G.CSRC/"jit_runtime.hpp").read_text()


def test_properties_on_every_finite_input(results):
    M.check_properties(results)


def test_vector_forms_go_through_the_scalar_ones(results):
    M.check_vector_forms(results)


def value(results, name, *operands):
    """the result at the first point whose operands are these, bit for bit"""
    case = M.BY_NAME[name]
    match = np.logical_and.reduce([M.bits(v) == M.bits(np.array([o], F))[0] for v, o in zip(M.operands_of(case), operands)])
    assert match.any(), (name, operands)
    return results[name][np.flatnonzero(match)[0]]


def test_known_values_and_the_oddities_that_stay(results):
    inf, nan = F(np.inf), M.QNAN
    # round: what floorf(x + 0.5f) got wrong, and the direction of exact halves (towards +inf, as the `builtins` golden was rendered)
    assert value(results, "round", F(0.49999997)) == 0 and value(results, "round", F(-0.49999997)) == 0
    assert value(results, "round", F(2.0**23 + 1)) == F(2.0**23 + 1) and value(results, "round", F(-2.0**23 - 1)) == F(-2.0**23 - 1)
    assert value(results, "round", F(2.0**23 - 0.5)) == F(2.0**23) and value(results, "round", F(-2.0**23 + 0.5)) == F(-2.0**23 + 1)
    assert [value(results, "round", F(v)) for v in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5)] == [1, 2, 3, 0, -1, -2]
    assert [value(results, "roundEven", F(v)) for v in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5)] == [0, 2, 2, 0, -2, -2]
    # int / uint: NaN -> 0, saturating
    for x, i, u in ((nan, 0, 0), (inf, 2**31 - 1, 2**32 - 1), (-inf, -2**31, 0), (F(2.0**31), 2**31 - 1, 2**31), (F(2.0**32), 2**31 - 1, 2**32 - 1),
                    (F(-2.0**31), -2**31, 0), (F(-2.5), -2, 0), (F(2.0**31 - 128), 2**31 - 128, 2**31 - 128), (F(2.0**32 - 256), 2**31 - 1, 2**32 - 256)):
        assert int(value(results, "int.high", x))*65536 + int(value(results, "int.low", x)) == i, x
        assert int(value(results, "uint.high", x))*65536 + int(value(results, "uint.low", x)) == u, x
    # beyond the reach of sfmath's reduction: bounded, and NaN only for what is not a number
    x = M.operands_of(M.BY_NAME["sin"])[0]
    far = np.isfinite(x) & (np.abs(x) > M.SINCOS_REACH)
    assert far.sum() > 6000 and np.abs(x[far]).max() == M.FLT_MAX
    for name in ("sin", "cos"):
        assert np.isfinite(results[name][far]).all() and np.abs(results[name][far]).max() <= 1 and results[name][far].std() > 0.5
        assert np.isnan(value(results, name, inf)) and np.isnan(value(results, name, nan))
    # pinned, not fixed: the cancellation of sinh and tanh around zero …
    assert value(results, "sinh", F(2.0**-25)) == 0 and value(results, "sinh", F(-2.0**-25)) == 0
    assert abs(float(value(results, "sinh", F(1e-4))) - 1e-4) < 2.0**-24 and abs(float(value(results, "sinh", F(1e-4)))/1e-4 - 1) > 1e-5
    assert abs(float(value(results, "tanh", F(1e-4))) - 1e-4) < 2.0**-24
    # … their overflow before the halving, atan of two infinities, a NaN that min/max drop, and pow where it is not IEEE's
    assert value(results, "sinh", F(89.0)) == inf and value(results, "cosh", F(89.0)) == inf and np.sinh(89.0) < M.FLT_MAX
    assert np.isnan(value(results, "atan2", inf, inf)) and np.isnan(value(results, "atan2", -inf, inf))
    assert value(results, "atan2", nan, F(0.0)) == 0
    assert value(results, "atan2", F(0.0), F(0.0)) == 0 and value(results, "atan2", F(1.0), F(0.0)) == F(np.pi/2)
    assert np.isnan(value(results, "pow", inf, F(0.0))) and np.isnan(value(results, "pow", F(-1.0), F(0.5)))
    assert value(results, "pow", F(0.0), F(0.0)) == 1 and value(results, "pow", F(0.0), F(2.5)) == 0 and value(results, "pow", F(0.0), F(-1.0)) == inf
    assert value(results, "pow", F(1.0), F(2.5)) == 1
    # fract reaches 1 just below zero; mod by zero and smoothstep between equal edges are what their formulas give
    assert value(results, "fract", -M.SUB_MIN) == 1 and value(results, "fract", F(-0.0)) == 0
    assert np.isnan(value(results, "mod", F(1.0), F(0.0))) and np.isnan(value(results, "smoothstep", F(1.0), F(1.0), F(1.0)))


def test_library_and_translated_kernels_compile_the_header_alike():
    """The restated kernels (csrc/Makefile) and the run-time translated ones (glsl2hip.FLAGS) include the same sfmath.hpp: the same
    floating-point switches on both, or the same source gives other bits"""
    makefile = (G.CSRC/"Makefile").read_text()
    flags = re.search(r"^FLAGS\s*=\s*((?:.*\\\n)*.*)$", makefile, re.M).group(1).replace("\\\n", " ").split()
    for switch in ("-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-fno-gpu-flush-denormals-to-zero", "-fno-slp-vectorize"):
        assert switch in flags, f"csrc/Makefile lacks {switch}"
        assert switch in G.FLAGS, f"glsl2hip.FLAGS lacks {switch}"
    for loosened in ("-ffast-math", "-ffp-contract=fast", "-ffp-contract=on", "-fgpu-flush-denormals-to-zero", "-Ofast", "-funsafe-math-optimizations"):
        assert loosened not in flags and loosened not in G.FLAGS, loosened
