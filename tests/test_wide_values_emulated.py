"""Wide terms and clocks on the EMULATED device (CPU; tests/host_device.py): the small cases of tests/test_wide_values.py -
the engine's own translation unit compiled for the host: the kernels as written (the timers' two 32-bit halves, the
feed's shadow, the vote mail's words, the device clock of the replayed rounds) and the host code around them."""
import host_device


def test_wide_values_small_cases_on_the_emulated_device():
    r = host_device.run_pytest(["tests/test_wide_values.py", "-m", "gpu", "-k", "small"])  # (with graphs: the replayed rounds advance the device clock, jg_kernels.h JgClock)
    tail = r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and " failed" not in r.stdout, tail[-800:]
