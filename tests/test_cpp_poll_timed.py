"""Build and run tests/cpp/test_poll_timed.cpp against the HIP engine: two worlds of three BatchedRafts exchange the same
messages while one broker's inbound traffic is withheld; each broker of one world is asked with the C++ watch calls
(watch_replicas_timed among them), its twin in the other with ONE BatchedRaft::poll carrying the clock (jg_poll.clock, ABI
v20) - the sample that starts the clocks, the window, the expiry and the rejoin - and everything returned is equal byte for
byte."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_poll_timed.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_poll_timed")


def compile_poll_timed_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_poll_timed_compiles():
    """CPU: the program and BatchedRaft::poll with a clock compile and link against the C ABI"""
    compile_poll_timed_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_poll_timed_equals_the_separate_calls_on_a_twin():
    compile_poll_timed_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "poll timed ok" in r.stdout
