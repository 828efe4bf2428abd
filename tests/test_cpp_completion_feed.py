"""Build and run tests/cpp/test_completion_feed.cpp against the HIP engine: three BatchedRafts in one jg_dense_cluster run
rounds on the device, which queue no FSM rows; each leader registers a waiter per appended id from its commit feed and every
request is answered exactly once through BatchedRaft::watch_completions (ABI v22)."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_completion_feed.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_completion_feed")


def compile_feed_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_completion_feed_compiles():
    """CPU: the program and BatchedRaft::open_waiters / await_blocks / watch_completions compile and link against the C ABI"""
    compile_feed_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_every_request_is_answered_once():
    compile_feed_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "completion feed ok" in r.stdout
