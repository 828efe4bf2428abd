"""Withdrawing waiters (jg_engine_await_cancel, ABI v24) on the EMULATED device (CPU; tests/host_device.py): the small cases of
tests/test_await_cancel.py and tests/test_node_await_cancel.py - the host code (the keys copied, checked, sorted, staged into
the engine's staging or behind an awaited step's rows; the shards' sum; the header block's marked word) and the mark pass
with both of its searches, rule 0 of the verdict and the chain of an awaited step as written, against numpy and against a
twin that steps synchronously, registers, cancels and watches."""
import host_device
import pytest


@pytest.mark.parametrize("module", ["test_await_cancel", "test_node_await_cancel"])
def test_await_cancel_small_cases_on_the_emulated_device(module):
    r = host_device.run_pytest([f"tests/{module}.py", "-m", "gpu", "-k", "small"], env=dict(JG_NO_GRAPH="1"))
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
