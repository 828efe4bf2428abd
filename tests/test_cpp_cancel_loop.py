"""Build and run tests/cpp/test_cancel_loop.cpp against the HIP engine: the awaited loop of tests/cpp/test_awaited_loop.cpp
with tokens that carry a connection id, a third of the connections closing mid-run through BatchedEventLoop::cancel_tokens
(jg_node_await_request.cancel_keys, ABI v24) - every token arrives at the sink exactly once, a closed connection's outstanding
tokens as JG_DONE_CANCELLED and none of them applied afterwards, and the table ends empty."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_cancel_loop.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_cancel_loop")


def compile_cancel_loop_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_cancel_loop_compiles():
    """CPU: the program, BatchedRaft::cancel_waiters, the request's cancel fields and BatchedEventLoop::cancel_tokens compile
    and link against the C ABI"""
    compile_cancel_loop_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_cancel_loop_every_token_once():
    compile_cancel_loop_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cancel loop ok" in r.stdout
