"""Build and run tests/cpp/test_replica_feed.cpp against the HIP engine: three BatchedRafts elect leaders and replicate
clients' appends through the wire; one broker's inbound traffic is withheld, and every other leader's feed
(BatchedRaft::watch_replicas, ABI v15) reports that broker's slot leaving the in-sync set of each partition it leads while
its census names the slot in out_of_sync; traffic resumes and the feed reports it rejoining."""
import os
import subprocess

import pytest

from josefine_amd.build import CSRC, build_hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_replica_feed.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "test_replica_feed")


def compile_feed_test():
    build_hip()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, SRC, f"-L{CSRC}", "-ljosefine_gpu",
                    f"-Wl,-rpath,{CSRC}", "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_cpp_replica_feed_compiles():
    """CPU: the program and BatchedRaft::watch_replicas / replication_census / isr_nodes compile and link against the C ABI"""
    compile_feed_test()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_cpp_leaders_report_the_withheld_broker_leaving_and_rejoining():
    compile_feed_test()
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "replica feed ok" in r.stdout
