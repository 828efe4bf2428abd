"""k_lookup_kept<R> - the lookup behind a kept node step (jg_lookup.h) - against k_lookup<R> of the same build, from the
compiler's resource report (no GPU: hipcc cross-compiles): the same body under one scalar load of the gate, so no scratch and
k_lookup's own registers plus the gate's handful.  The gate's verdict is a scalar; what it can cost in vector registers is
the header word's store by one lane - a 64-bit address and the value - so the handful is 4."""
import pytest

from test_kernel_resources import report  # noqa: F401 (the fixture: one run of profiles/kernel_resources.sh)

GATE_VGPRS = 4


@pytest.mark.parametrize("R", range(1, 9))
def test_the_kept_lookup_costs_what_the_lookup_costs(report, R):  # noqa: F811
    plain, kept = report[f"void k_lookup<{R}>"], report[f"void k_lookup_kept<{R}>"]
    assert plain["scratch"] == 0 and kept["scratch"] == 0, (plain, kept)
    assert kept["vgprs"] <= plain["vgprs"] + GATE_VGPRS, (plain, kept)
    assert kept["waves"] >= plain["waves"], (plain, kept)
