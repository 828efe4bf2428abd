"""The completion feed (jg_engine_await_open / _await_blocks / _watch_completions) on the EMULATED device (CPU;
tests/host_device.py): the small cases of tests/test_completion_feed.py - the host code, the count / scan / write passes with
the verdict rules and the compaction as written, against numpy over the engine's own columns and the reference's Driver."""
import host_device


def test_completion_feed_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_completion_feed.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
