"""Build and run tests/cpp/test_hosted_loop.cpp against the HIP engine: ONE BatchedEventLoop with two ticks in flight that
closes and opens partitions every tick (BatchedEventLoop::close_async / open_async: jg_step_node_hosted /
jg_node_hosting_view, ABI v26) over a few thousand partitions - every sink is called exactly once, in request order, a
refused set leaves the other one applied, a reopened partition elects again, and the engine's hosted set ends as the host's
own bookkeeping."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_hosted_loop.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_hosted_loop")


def compile_hosted_loop_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_hosted_loop_compiles():
    """CPU: the program, BatchedRaft::step_node_hosted / node_hosting and BatchedEventLoop::open_async / close_async compile
    and link against the C ABI"""
    compile_hosted_loop_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_hosted_loop_every_request_once_in_order():
    compile_hosted_loop_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hosted loop ok" in r.stdout
