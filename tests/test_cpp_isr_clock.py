"""Build and run tests/cpp/test_isr_clock.cpp against the HIP engine: three BatchedRafts exchange messages; while one
broker's inbound traffic is withheld, the C++ timed replica feed (BatchedRaft::watch_replicas_timed, ABI v19) keeps that
broker's slot in the in-sync set of each partition the others lead until it has been behind for longer than the window of the
caller's clock, reports it leaving with the first sample past it, and reports it rejoining once the traffic has resumed."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_isr_clock.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_isr_clock")


def compile_isr_clock_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_isr_clock_compiles():
    """CPU: the program and BatchedRaft::watch_replicas_timed compile and link against the C ABI"""
    compile_isr_clock_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_isr_clock_leaves_by_time_and_rejoins():
    compile_isr_clock_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "isr clock ok" in r.stdout
