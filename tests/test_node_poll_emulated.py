"""A poll behind a kept node step (jg_step_node_polled, ABI v21) on the EMULATED device (CPU; tests/host_device.py): the small
cases of tests/test_node_poll.py - the host code of the polled step (the request copied, the chain queued behind the step and
once more behind the catch-up pass, the header block, the landing areas, the view) and the gated passes as written, against a
twin that steps synchronously and polls."""
import host_device


def test_node_poll_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_node_poll.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
