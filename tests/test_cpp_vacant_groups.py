"""Build and run tests/cpp/test_vacant_groups.cpp against the HIP engine: three BatchedRafts start with every slot vacant
(JG_CFG_START_VACANT), open one partition at runtime on all three (jg_engine_open_groups, ABI v13), elect and commit; then
one of them closes it - its slot emits nothing more while the other two keep committing."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_vacant_groups.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_vacant_groups")


def compile_vacant_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_vacant_groups_compiles():
    """CPU: the program and BatchedRaft::open_groups / close_groups / vacant_groups compile and link against the C ABI"""
    compile_vacant_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_partitions_opened_and_closed_at_runtime():
    compile_vacant_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "vacant groups ok" in r.stdout
