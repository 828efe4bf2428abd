"""Wide terms and clocks on the CPU (tests/wide_values.py): first the two restatements of the reference against each other
- the C++ oracle and tests/ref_py, which compute in uint64_t and in Python ints - then the DEVICE SOURCE compiled for the
host (tests/host_compiled.py: the general state machine, the dense leader and follower bodies, the slow bodies, the node
step's passes) against the oracle, from clocks at 2^32 - 450, wall-clock milliseconds and 2^63 - 450 and terms at 2^32 - 3,
(7 << 32) + 5 and 2^63 - 3."""
import numpy as np
import pytest

from josefine_amd import capi
from fuzz import random_batch, random_batch_aware
from host_compiled import HostCompiled
from oracle_lib import oracle_engine
from parity import compare_drains, compare_snapshots
from ref_py.engine import RefEngine
from wide_values import (BOUND, C32, CWRAP, PAIR_IDS, PAIRS, T32, follower_half_case, leader_half_case, node_step_case, raise_clock, raise_term,
                         unvoted_at)


def _streams(make, R, base, term, stream, seed, budget=False):
    """the blind and the live command streams of tests/fuzz.py from a wide clock and term: every group gets the Heartbeat at
    `term` (groups 0 mod 2) or reaches it without a vote (groups 1 mod 2: the ones that can campaign, so that candidates
    and leaders appear at wide terms)"""
    G, steps, rows = 200, 40, 800
    rng = np.random.default_rng(seed)
    slots = rng.integers(0, R, G).astype(np.uint8)
    kw = dict(seed=R, self_slots=slots, flags=capi.CFG_SEPARATE_COMMIT_KEY if R == 5 else 0, election_timeout_ms=(300, 700))
    dev, ora = make(G, R, **kw), oracle_engine(G, R, **kw)
    g = np.arange(G)
    for e in (dev, ora):
        raise_clock([e], base)
        unvoted_at([e], term, base, g[g % 2 == 1])
        raise_term([e], term, None, base, g[g % 2 == 0])
    compare_snapshots(dev, ora, "wide set-up")
    compare_drains(dev, ora, "wide set-up")
    assert (ora.read("term") == np.uint64(term)).all() and (ora.read("election_time") == np.uint64(base)).all()
    lim = np.full(G, capi.CHAIN_WINDOW - 2) if budget else None  # (the engine's segment window; the restatements have none)
    now = base
    led = campaigns = 0
    crossed = False
    for s in range(steps):
        b = random_batch(rng, ora, rows, foreign_voters=True, budget=lim) if stream == "blind" else random_batch_aware(rng, ora, rows)
        now += int(rng.integers(0, 300))
        for e in (dev, ora):
            e.submit_columns(**b)
            e.step(now)
        compare_drains(dev, ora, f"R={R} step {s}")
        if s % 8 == 7 or s == steps - 1:
            compare_snapshots(dev, ora, f"R={R} step {s}")
        up = ora.read("term") > np.uint64(term)
        led = max(led, int(((ora.read("role") == capi.ROLE_LEADER) & up).sum()))
        campaigns = max(campaigns, int(((ora.read("role") != capi.ROLE_FOLLOWER) & up).sum()))
        crossed |= bool((ora.read("term") >= np.uint64(BOUND)).any())
    assert dev.counters()["decisions"] == ora.counters()["decisions"] > 0
    # campaigns above the term base, and under the live stream leaders: elected at wide terms, not after a restart
    assert campaigns > 0 and (led > 0 or stream == "blind"), (campaigns, led)
    if base == C32:
        assert int(ora.read("election_time").max()) >= BOUND
    if term == T32:  # (the live stream restarts what it can: most groups end at small terms)
        assert crossed


# ---- 1a: the oracle against tests/ref_py -------------------------------------------------------------------------------
@pytest.mark.parametrize("base,term", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("R", [3, 5])
@pytest.mark.parametrize("stream", ["blind", "live"])
def test_the_two_restatements_agree_at_wide_values(stream, R, base, term):
    _streams(RefEngine, R, base, term, stream, seed=31000 + R)


# ---- 1b: the device source compiled for the host -----------------------------------------------------------------------
@pytest.fixture(params=["dense kernels' own logic, then the slow bodies", "slow bodies only"])
def dense_path(request, monkeypatch):
    """as tests/test_host_compiled_state_machine.py: the dense halves served the way the device serves them, and with every
    group handed to the slow bodies"""
    monkeypatch.setattr(HostCompiled, "fast", request.param.startswith("dense"))


@pytest.mark.parametrize("base,term", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("R", [3, 5])
@pytest.mark.parametrize("stream", ["blind", "live"])
def test_host_compiled_state_machine_at_wide_values(stream, R, base, term):
    _streams(HostCompiled, R, base, term, stream, seed=33000 + R, budget=True)


@pytest.mark.parametrize("base,term", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("R", [3, 5])
def test_host_compiled_leader_half_at_wide_values(dense_path, R, base, term):
    leader_half_case(HostCompiled, oracle_engine, R, base, term, "last")


@pytest.mark.parametrize("base,term", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("R", [3, 5])
def test_host_compiled_follower_half_at_wide_values(dense_path, R, base, term):
    follower_half_case(HostCompiled, oracle_engine, R, base, term, "last")


@pytest.mark.parametrize("R", [3, 5])
def test_host_compiled_halves_translate_across_the_wrap(dense_path, R):
    """the device source at now + 2^64 - 450, the oracle at now: every column equal, the timers equal less the shift"""
    leader_half_case(HostCompiled, oracle_engine, R, CWRAP, T32, "last", ref_base=0)
    follower_half_case(HostCompiled, oracle_engine, R, CWRAP, T32, "last", ref_base=0)


@pytest.mark.parametrize("base,term", PAIRS[:2], ids=PAIR_IDS[:2])
@pytest.mark.parametrize("R", [3, 5])
def test_host_compiled_node_step_at_wide_values(R, base, term):
    node_step_case(HostCompiled, oracle_engine, R, base, term)


def test_the_reference_restatements_run_the_dense_halves_at_wide_values():
    """the halves' cases on tests/ref_py against the oracle: the conditions they assert hold on an independent reading too"""
    leader_half_case(RefEngine, oracle_engine, 3, C32, T32, "mixed")
    follower_half_case(RefEngine, oracle_engine, 3, C32, T32, "mixed")
