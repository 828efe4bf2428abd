"""The replication feed and its census (jg_engine_watch_replicas / jg_engine_replication_census) on the EMULATED device
(CPU; tests/host_device.py): the small cases of tests/test_replica_feed.py - the host code, the count / scan / write passes
with the packed word's decode, and the census reduction as written, against numpy over the engine's own columns, ref_py and
unwatched twins."""
import host_device


def test_replica_feed_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_replica_feed.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
