"""k_groups_check_kept / k_groups_open_kept / k_groups_close_kept - hosting behind a kept node step (jg_hosting.h) - against
k_groups_check / k_groups_open / k_groups_close of the same build, from the compiler's resource report (no GPU: hipcc
cross-compiles): the same bodies under one scalar load of the gate, so no scratch and the plain kernel's own registers plus
the gate's handful.  The gate's verdict is a scalar; what it can cost in vector registers is the header word's store by one
lane - a 64-bit address and the value, and in the write kernels the error word read for it - so the handful is 4."""
import pytest

from test_kernel_resources import report  # noqa: F401 (the fixture: one run of profiles/kernel_resources.sh)

GATE_VGPRS = 4


@pytest.mark.parametrize("kernel", ["check", "open", "close"])
def test_the_kept_hosting_kernels_cost_what_the_plain_ones_cost(report, kernel):  # noqa: F811
    plain, kept = report[f"k_groups_{kernel}"], report[f"k_groups_{kernel}_kept"]
    assert plain["scratch"] == 0 and kept["scratch"] == 0, (plain, kept)
    assert kept["vgprs"] <= plain["vgprs"] + GATE_VGPRS, (plain, kept)
    assert kept["waves"] >= plain["waves"], (plain, kept)
