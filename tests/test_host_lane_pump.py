"""
The copier loop of the read-out ring, the peer copier and the shared-memory publisher (csrc/lane_pump.hpp), without a GPU:
tests/lane_pump_check.cpp drives it with lanes that land when the case says so, as a process of its own, once under the thread
sanitizer and once under the address and undefined-behaviour sanitizers.
"""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

SANITIZERS = {
    "thread": (["-fsanitize=thread", "-static-libtsan"], ("-ltsan", "libtsan")),
    "address": (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"], ("-lasan", "-lubsan", "libasan", "libubsan")),
}


@pytest.mark.parametrize("sanitizer", sorted(SANITIZERS))
def test_the_lane_pump_alone(sanitizer, tmp_path):
    """Rotation over 1, 2 and 4 lanes, reports in issue order or ahead of their turn, a job that is not ready or not issued under both
    answers of the owner, a failed copy, a job that takes no lane, both stops, and 2 000 jobs against copies landing in random order"""
    compiler = shutil.which("g++")
    if compiler is None:
        pytest.skip("no g++")
    flags, runtime = SANITIZERS[sanitizer]
    program = tmp_path/"lane_pump_check"
    built = subprocess.run([compiler, "-std=c++17", "-O1", "-g", *flags,              # the runtimes in the program itself: it needs nothing from its environment
                            "-I", str(ROOT/"shaderflow_amd"/"csrc"), str(ROOT/"tests"/"lane_pump_check.cpp"), "-o", str(program), "-lpthread"],
                           capture_output=True, text=True)
    if built.returncode and any(word in built.stderr for word in runtime):
        pytest.skip("g++ lacks the sanitizer runtime")
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(program)], capture_output=True, text=True, timeout=600)
    assert ran.returncode == 0 and not ran.stderr, ran.stdout + ran.stderr
    lines = ran.stdout.splitlines()
    assert len(lines) == 18 and all(line.startswith("ok ") for line in lines), ran.stdout
