"""jg_engine_read_chains on the EMULATED device (CPU; tests/host_device.py): the small cases of tests/test_read_chains.py -
the read's host code, its group passes, scans and row pass as written, against ref_py's sled trees."""
import host_device


def test_read_chains_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_read_chains.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
