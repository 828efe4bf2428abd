"""One poll per tick (jg_engine_poll) on the EMULATED device (CPU; tests/host_device.py): the small cases of
tests/test_poll.py - the host code, the fused count pass, the one scan launch over the wanted feeds' tile counts, the
feeds' own write passes and the census kernels behind it as written, against the separate calls on a twin."""
import host_device


def test_poll_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_poll.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
