"""Completions behind a kept node step (jg_step_node_awaited, ABI v23) on the EMULATED device (CPU; tests/host_device.py): the
small cases of tests/test_node_await.py - the host code of the awaited step (the request and its rows copied, the bound, the
head written from the host's values, the chain queued behind the step and once more behind the catch-up pass, the header
block, the landing area, the view that refreshes n and cur) and the kernels that read the table's head as written, against a
twin that steps synchronously, registers and watches."""
import host_device


def test_node_await_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_node_await.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
