"""Build and run tests/cpp/test_move_groups.cpp against the HIP engine: a 3-node cluster through the C++ host mirror
(josefine_amd/host/raft_handle.hpp) commits, its leader's instance and store move to a fresh BatchedRaft
(jg_engine_export_groups / jg_engine_import_groups, ABI v12), and the cluster keeps committing with the same leader and
term - no election (contrast tests/cpp/test_restart_open.cpp)."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_move_groups.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_move_groups")


def compile_move_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_move_groups_compiles():
    """CPU: the program and BatchedRaft::export_groups / import_groups compile and link against the library's C ABI"""
    compile_move_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_live_hand_over_keeps_leader_and_term():
    compile_move_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "move groups ok" in r.stdout
