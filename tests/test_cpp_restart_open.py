"""Build and run tests/cpp/test_restart_open.cpp against the HIP engine: a 3-node cluster through the C++ host mirror
(josefine_amd/host/raft_handle.hpp) commits, its process dies, and BatchedRaft::open (jg_engine_load_chains, ABI v10)
brings it back on the stores' raw bytes."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_restart_open.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_restart_open")


def compile_restart_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_restart_open_compiles():
    """CPU: the program and BatchedRaft::open compile and link against the library's C ABI"""
    compile_restart_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_broker_restart_on_its_stores():
    compile_restart_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "restart open ok" in r.stdout
