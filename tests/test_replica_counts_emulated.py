"""Every replica count at the edge of its lag field on the EMULATED device (CPU; tests/host_device.py): the small cases of
tests/test_replica_counts.py - the ladder at R = 4, 6, 7, 8 and the node steps at R = 6 and 8 - through the engine's own
translation unit compiled for the host: the templates on R, the generic readers of the packed word and their host code as
written.  (The exact decision counters are not compared there: JG_EMULATED_DEVICE.)"""
import host_device


def test_replica_counts_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_replica_counts.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
