"""Build and run tests/cpp/test_awaited_loop.cpp against the HIP engine: ONE BatchedEventLoop with two ticks in flight and a
completion request attached to every tick's step (BatchedEventLoop::set_completions: jg_step_node_awaited /
jg_node_await_view, ABI v23) over a few thousand partitions - every Notify row of a tick becomes a waiter, every token arrives
at the sink exactly once, applied, in registration order per partition, and the table ends empty."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_awaited_loop.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_awaited_loop")


def compile_awaited_loop_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_awaited_loop_compiles():
    """CPU: the program, BatchedRaft::step_node_awaited / node_completions and BatchedEventLoop::set_completions compile and
    link against the C ABI"""
    compile_awaited_loop_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_awaited_loop_every_token_once():
    compile_awaited_loop_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "awaited loop ok" in r.stdout
