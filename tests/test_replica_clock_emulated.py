"""Time-based in-sync sets (jg_engine_watch_replicas_timed) on the EMULATED device (CPU; tests/host_device.py): the small
cases of tests/test_replica_clock.py - the host code, the count pass that advances the clocks, the scan and the write pass
as written, against the numpy statement of the rule."""
import host_device


def test_replica_clock_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_replica_clock.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
