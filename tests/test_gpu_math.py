"""
The GLSL built-ins of csrc/jit_runtime.hpp value by value ON THE DEVICE: the probe of tests/math_cases.py, translated and compiled for
gfx950 the way every fragment outside the registry is, evaluated over the same inputs as tests/test_host_math.py and held to
(1) the operands it was fed, (2) the x86 host build's bits, (3) the references, bounds and properties of math_cases on its own,
(4) the oracle's bits.
"""
import numpy as np
import pytest

from oracle import binding as O
from shaderflow_amd import _native as N
from tests import math_cases as M
from tests.helpers import Gpu
from tests.test_gpu_translated import load
from tests.test_host_math import host_evaluation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def evaluation():
    gpu = Gpu()
    prog, _ = load(gpu, M.probe_glsl(), M.PROBE_UNIFORMS)
    gpu.set_uniforms(prog, O.default_uniforms(M.WIDTH, M.HEIGHT))
    uploaded = {}

    def render(group, texels):
        key = texels.ctypes.data
        if key not in uploaded:                                    # one upload per array of operands, shared by its groups (the
            uploaded[key] = (gpu.texture(texels, "nearest", False, False), texels)      # array is kept: its address is the key)
        assert gpu.set_values(prog, "group", group, integer=True)
        assert gpu.bind(prog, "operands", uploaded[key][0])
        return gpu.render(prog, M.WIDTH, M.HEIGHT, comps=4, dtype=np.float32)
    try:
        yield M.evaluate(render)
    finally:
        N.check(gpu.lib.sfx_program_destroy(prog))
        gpu.close()


@pytest.fixture(scope="module")
def results(evaluation):
    return evaluation[0]


def test_device_returns_its_operands_bit_for_bit(evaluation):
    M.check_echo(evaluation[1])


def test_device_equals_the_host_build_bit_for_bit(results):
    host, _ = host_evaluation()
    M.check_same(results, host, "device (got) against the x86 host build (want)")


def test_device_equals_the_oracle_bit_for_bit(results):
    M.check_oracle(results)


def test_device_against_the_references_on_its_own(results):
    M.check_exact(results)
    M.check_approx(results)
    M.check_circular(results)
    M.check_properties(results)
    M.check_vector_forms(results)
