"""Poll under the time rule (jg_poll.clock, ABI v20) on the EMULATED device (CPU; tests/host_device.py): the small cases of
tests/test_poll_timed.py - the host code, the timed fused count pass with the clocks it advances, k_isrc_write behind it and
the sharded sizing pass as written, against the separate calls on a twin."""
import host_device


def test_poll_timed_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_poll_timed.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
