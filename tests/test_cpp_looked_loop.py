"""Build and run tests/cpp/test_looked_loop.cpp against the HIP engine: ONE BatchedEventLoop with two ticks in flight and a
point query asked every tick (BatchedEventLoop::lookup_async: jg_step_node_looked / jg_node_lookup_view, ABI v25) over a few
thousand partitions - every sink is called exactly once, in request order, no row is older than what the loop's own sinks
had shown of its partition when the request was made, and a last request equals the synchronous BatchedRaft::lookup."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_looked_loop.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_looked_loop")


def compile_looked_loop_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_looked_loop_compiles():
    """CPU: the program, BatchedRaft::step_node_looked / node_lookup and BatchedEventLoop::lookup_async compile and link
    against the C ABI"""
    compile_looked_loop_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_looked_loop_every_request_once_in_order():
    compile_looked_loop_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "looked loop ok" in r.stdout
