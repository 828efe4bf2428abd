"""Build and run tests/cpp/test_lookup_groups.cpp against the HIP engine: a BatchedRaft with leaders, informed followers,
candidates and closed slots answers BatchedRaft::lookup (ABI v16) for a list with repeats and for a range, and every row
equals jg_read_state at the listed index, field by field."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_lookup_groups.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_lookup_groups")


def compile_lookup_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_lookup_groups_compiles():
    """CPU: the program and BatchedRaft::lookup compile and link against the C ABI"""
    compile_lookup_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_lookup_rows_equal_read_state_at_the_listed_indices():
    compile_lookup_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lookup groups ok" in r.stdout
