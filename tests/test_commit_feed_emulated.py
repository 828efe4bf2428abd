"""The commit feed (jg_engine_watch_commits) on the EMULATED device (CPU; tests/host_device.py): the small cases of
tests/test_commit_feed.py - the host code, the count / scan / write passes with the decode of a leader's commit, and the
backlog reduction as written, against numpy over the engine's own columns, command-driven and unwatched twins."""
import host_device


def test_commit_feed_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_commit_feed.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
