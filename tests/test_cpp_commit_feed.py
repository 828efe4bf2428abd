"""Build and run tests/cpp/test_commit_feed.cpp against the HIP engine: three BatchedRafts in one jg_dense_cluster run
rounds on the device, which queue no FSM rows; each broker's set of applied block keys is advanced only from its commit
feed (BatchedRaft::watch_commits + as_fsm_rows, ABI v17) and ends as exactly the keys up to that broker's commit column."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_commit_feed.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_commit_feed")


def compile_feed_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_commit_feed_compiles():
    """CPU: the program and BatchedRaft::watch_commits / as_fsm_rows compile and link against the C ABI"""
    compile_feed_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_stores_advance_from_the_commit_feed_alone():
    compile_feed_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "commit feed ok" in r.stdout
