"""Build and run tests/cpp/test_read_chains.cpp against the HIP engine: a 3-node cluster through the C++ host mirror
(josefine_amd/host/raft_handle.hpp) commits, and each node's BatchedRaft::read_chains (jg_engine_read_chains, ABI v11)
must be its BlockStore - before and after BatchedRaft::open on the stores' raw bytes."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_read_chains.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_read_chains")


def compile_read_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_read_chains_compiles():
    """CPU: the program and BatchedRaft::read_chains compile and link against the library's C ABI"""
    compile_read_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_engine_chains_are_the_stores():
    compile_read_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "read chains ok" in r.stdout
