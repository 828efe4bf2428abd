"""Build and run tests/cpp/test_leader_feed.cpp against the HIP engine: three BatchedRafts host the same partitions and
elect a leader for each through the wire; every broker's feed (BatchedRaft::watch_leaders, ABI v14) then names the same
leader and term for it, exactly one reports SELF, the brokers' censuses add up, and after one broker closes its replica its
feed says VACANT."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_leader_feed.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_leader_feed")


def compile_feed_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_leader_feed_compiles():
    """CPU: the program and BatchedRaft::watch_leaders / census compile and link against the C ABI"""
    compile_feed_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_brokers_agree_on_every_partitions_leader():
    compile_feed_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "leader feed ok" in r.stdout
