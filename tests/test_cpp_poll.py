"""Build and run tests/cpp/test_poll.cpp against the HIP engine: two clusters of three BatchedRafts run the same rounds on
the device; each broker of one is asked with the three C++ watch calls and the two censuses, its twin in the other with ONE
BatchedRaft::poll (jg_engine_poll, ABI v18) - caps, peeks and a swap of the twins included - and everything returned is equal
byte for byte."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_poll.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_poll")


def compile_poll_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_poll_compiles():
    """CPU: the program and BatchedRaft::poll compile and link against the C ABI"""
    compile_poll_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_poll_equals_the_separate_calls_on_a_twin():
    compile_poll_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "poll ok" in r.stdout
