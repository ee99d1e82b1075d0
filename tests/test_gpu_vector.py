"""
The vector, matrix and integer built-ins of csrc/jit_runtime.hpp value by value ON THE DEVICE: the probes of tests/vector_cases.py,
translated and compiled for gfx950 the way every fragment outside the registry is, evaluated over the same inputs as
tests/test_host_vector.py and held to (1) the operands they were fed, (2) the x86 host build's bits on every point of every row,
(3) the restatements, the float64 witnesses and the inverse property on the device's own results.
"""
import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import _native as N
from tests import vector_cases as V
from tests.helpers import Gpu
from tests.test_gpu_translated import load
from tests.test_host_vector import host_evaluation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    """fragment -> ({row: results}, {set: echo}) from the gfx950 code object; each probe is compiled and evaluated once"""
    gpu = Gpu()
    programs, uploaded, done = [], {}, {}

    def evaluation(fragment):
        if fragment in done:
            return done[fragment]
        width, height = V.rows_of(fragment)[0].size
        prog, _ = load(gpu, V.probe_glsl(fragment), V.PROBE_UNIFORMS)
        programs.append(prog)
        gpu.set_uniforms(prog, O.default_uniforms(width, height))
        target = gpu.empty(width, height, 4, np.float32)           # one target for every render of the fragment

        def render(group, column, four, size):
            assert size == (width, height)
            for name, texels in zip(("opA", "opB", "opC", "opD"), four):
                key = texels.ctypes.data
                if key not in uploaded:                            # one upload per array of operands (kept: its address is the key)
                    uploaded[key] = (gpu.texture(texels, "nearest", False, False), texels)
                assert gpu.bind(prog, name, uploaded[key][0])
            assert gpu.set_values(prog, "group", group, integer=True) and gpu.set_values(prog, "column", column, integer=True)
            N.check(gpu.lib.sfx_render(prog, target, 0))
            return gpu.read(target, width, height, 4, np.float32)
        done[fragment] = V.evaluate(fragment, render)
        return done[fragment]
    try:
        yield evaluation
    finally:
        for prog in programs:
            N.check(gpu.lib.sfx_program_destroy(prog))
        gpu.close()


@pytest.mark.parametrize("fragment", V.FRAGMENTS)
def test_device_returns_its_operands_bit_for_bit(device, fragment):
    V.check_echo(device(fragment)[1])


@pytest.mark.parametrize("fragment", V.FRAGMENTS)
def test_device_equals_the_host_build_bit_for_bit(device, fragment):
    results = device(fragment)[0]
    host = host_evaluation(fragment)[0]
    assert set(results) == set(host) == {row.name for row in V.rows_of(fragment)}
    V.check_same(results, host, f"{fragment}: device (got) against the x86 host build (want)")


@pytest.mark.parametrize("fragment", V.FRAGMENTS)
def test_device_against_the_references_on_its_own(device, fragment):
    results = device(fragment)[0]
    V.check_exact(fragment, results)
    V.check_witness(fragment, results)
    if fragment == "matrix":
        V.check_inverse(results)
