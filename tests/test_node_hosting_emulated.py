"""Hosting behind a kept node step (jg_step_node_hosted, ABI v26) on the EMULATED device (CPU; tests/host_device.py): the small
cases of tests/test_node_hosting.py - the host code of the hosted step (the two sets checked and copied, the lists and own
slots staged, the check and write passes queued last behind the step under its gate and once more behind the catch-up pass,
the header words, what the rewrite owes the next step and not this one, the view) and the kept kernels as written, against a
twin that steps synchronously, closes and opens."""
import host_device


def test_node_hosting_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_node_hosting.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
