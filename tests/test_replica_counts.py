"""Every replica count held to the oracle at the edge of its lag field (tests/replica_counts.py): the ladder - climb to
BEHIND - 2, four one-block rungs over the edge, a quiet tick, a forged ack, the rejoin - for R = 2 .. 8 with mixed own slots
and for R = 4 and 7 with one own slot throughout, once more at R = 7 with the dense tick split over two streams, and ten
node steps under adversarial traffic at R = 2, 4, 6, 7, 8.  After every tick: every column and drained row against the
oracle, the replication feed at thresholds on both sides of BEHIND and its census against numpy, lookup with progress
heads, the commit feed, and a twin's poll against the separate calls.  The cases with `small` in their id also run on the
emulated device (tests/test_replica_counts_emulated.py).

Partitions that climb, per R: 2 at R = 2, 90 at R = 3, all 357 from R = 4 on (tests/replica_counts.py says why).
Measured on an MI355X, per case, the oracle's block-by-block appends included (they are most of the first two):
test_ladder 2-mixed 1.55 s, 3-mixed 0.97 s, 4-mixed 0.34 s, 4-uniform 0.35 s, 5-mixed 0.25 s, 6-mixed 0.25 s, 7-mixed
0.22 s, 7-uniform 0.24 s, 8-mixed 0.23 s; test_ladder_split_tick 0.21 s; test_node_steps 0.08 - 0.12 s each."""
import pytest

from josefine_amd import BatchedRaft
from oracle_lib import oracle_engine
from replica_counts import ladder, node_steps

pytestmark = pytest.mark.gpu

SMALL = (4, 6, 7, 8)
LADDERS = [pytest.param(R, "mixed", id=f"{'small-' if R in SMALL else ''}{R}-mixed") for R in range(2, 9)] + \
          [pytest.param(R, "uniform", id=f"{R}-uniform") for R in (4, 7)]


@pytest.mark.parametrize("R,layout", LADDERS)
def test_ladder(R, layout):
    ladder(BatchedRaft, oracle_engine, R, layout)


def test_ladder_split_tick(monkeypatch):
    """JG_DENSE_SPLIT_MIN=1 (read when an engine is created: tests/test_gpu_dense_split.py): at G = 357 the cut is 256 and
    the second range, on the second stream, is the ragged workgroup"""
    monkeypatch.setenv("JG_DENSE_SPLIT_MIN", "1")
    ladder(BatchedRaft, oracle_engine, 7, "mixed", twin=False)


@pytest.mark.parametrize("R", [pytest.param(R, id=f"{'small-' if R in (6, 8) else ''}{R}") for R in (2, 4, 6, 7, 8)])
def test_node_steps(R):
    node_steps(BatchedRaft, oracle_engine, R)
