"""Point queries behind a kept node step (jg_step_node_looked, ABI v25) on the EMULATED device (CPU; tests/host_device.py): the
small cases of tests/test_node_lookup.py - the host code of the looked step (the set checked and copied, the list staged,
the launch queued behind the step under its gate and once more behind the catch-up pass, the header words, the landing area
sized at entry, the view) and k_lookup_kept as written, against a twin that steps synchronously and looks up."""
import host_device


def test_node_lookup_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_node_lookup.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
