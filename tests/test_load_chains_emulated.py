"""jg_engine_load_chains on the EMULATED device (CPU; tests/host_device.py): the small cases of tests/test_load_chains.py -
the load's host code and its row / group passes as written, against ref_py's restart on the same trees."""
import host_device


def test_load_chains_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_load_chains.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
