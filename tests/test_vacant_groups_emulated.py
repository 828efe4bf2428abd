"""Vacant slots (jg_engine_open_groups / jg_engine_close_groups / jg_engine_list_groups) on the EMULATED device (CPU;
tests/host_device.py): the small cases of tests/test_vacant_groups.py - the host code, the check and write passes and the
list's stream compaction as written, against ref_py and control engines."""
import host_device


def test_vacant_groups_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_vacant_groups.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
