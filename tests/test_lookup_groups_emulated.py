"""Point queries (jg_engine_lookup_groups) on the EMULATED device (CPU; tests/host_device.py): the small cases of
tests/test_lookup_groups.py - the host code (the one-piece path, the device list's error word, the partition by shard and
the scatter back) and k_lookup's decode as written, against e.read(...) indexed with the list and the leadership view."""
import host_device


def test_lookup_groups_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_lookup_groups.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
