"""Build and run tests/cpp/test_polled_loop.cpp against the HIP engine: ONE BatchedEventLoop with two ticks in flight and a
poll attached to every tick's step (BatchedEventLoop::set_poll: jg_step_node_polled / jg_node_poll_view, ABI v21) over a few
thousand partitions - the sink's commit rows, concatenated, reproduce every partition's final (commit, head) from genesis, and
its leader rows end at the view the engine holds."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_polled_loop.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_polled_loop")


def compile_polled_loop_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_polled_loop_compiles():
    """CPU: the program, BatchedRaft::step_node_polled / node_poll and BatchedEventLoop::set_poll compile and link against the
    C ABI"""
    compile_polled_loop_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_polled_loop_feeds_reproduce_the_state():
    compile_polled_loop_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "polled loop ok" in r.stdout
