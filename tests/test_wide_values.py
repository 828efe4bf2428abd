"""Wide terms and clocks on the device (tests/wide_values.py): every entry point that carries a 64-bit term or clock - the
dense halves, the node step through both bus formats, the routed and the replayed cluster rounds, the readers - from clocks
at 2^32 - 450 (the boundary is crossed inside the run), wall-clock milliseconds and 2^63 - 450 and terms at 2^32 - 3,
(7 << 32) + 5 and 2^63 - 3, against the oracle; and, shifted by 2^64 - 450, as a translation of the run at small clocks.
The cases with `small` in their id also run on the emulated device (tests/test_wide_values_emulated.py)."""
import numpy as np
import pytest

from josefine_amd import BatchedRaft, capi
from dense_node import DenseCluster
from oracle_lib import oracle_engine
from parity import compare_snapshots
from wide_values import (BOUND, C32, C63, CWRAP, M64, PAIR_IDS, PAIRS, T32, T63, check_cluster_drains, compare_shifted, follower_half_case,
                         leader_half_case, node_step_case, raise_clock, raise_term, routed_cluster_case, sides, wide_cluster, wide_cluster_nodes)

pytestmark = pytest.mark.gpu

SMALL_PAIRS = [pytest.param(b, t, id=f"small-{i}") for (b, t), i in zip(PAIRS, PAIR_IDS)]
LAYOUT = {3: "mixed", 5: "last"}


# ---- 2. the dense halves -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,term", SMALL_PAIRS)
@pytest.mark.parametrize("R", [3, 5])
def test_dense_leader_half(R, base, term):
    leader_half_case(BatchedRaft, oracle_engine, R, base, term, LAYOUT[R])


@pytest.mark.parametrize("base,term", SMALL_PAIRS)
@pytest.mark.parametrize("R", [3, 5])
def test_dense_follower_half(R, base, term):
    follower_half_case(BatchedRaft, oracle_engine, R, base, term, LAYOUT[R])


# ---- 3. the node step through both bus formats -------------------------------------------------------------------------
@pytest.mark.parametrize("base,term", SMALL_PAIRS[:2])
@pytest.mark.parametrize("keep", [False, True], ids=["one-step", "two-in-flight"])
@pytest.mark.parametrize("compact", [False, True], ids=["plain", "packed-id32"])
@pytest.mark.parametrize("R", [3, 5])
def test_node_step(R, compact, keep, base, term):
    node_step_case(BatchedRaft, oracle_engine, R, base, term, compact=compact, keep=keep)


# ---- 4. clusters -------------------------------------------------------------------------------------------------------
# (the routed cases the emulated device runs as well - `small` - are one diagonal of leadership x transport x base, at 12
# rounds: a routed round costs it seconds; the device runs every combination)
def _routed_params():
    out = []
    for any_leader in (False, True):
        for words in (False, True):
            for (base, term), name in (((C32, T32), "c32-t32"), ((C63, T63), "c63-t63")):
                what = f"{'any-leader' if any_leader else 'lead0'}-{'vote-words' if words else 'rows'}-{name}"
                diagonal = (any_leader == words) == (base == C32)
                out.append(pytest.param(3, 192, 12, 25, any_leader, words, base, term, id=("small-3-" if diagonal else "3-") + what))
                out.append(pytest.param(3, 192, 40, 25, any_leader, words, base, term, id="3-40-rounds-" + what))
                out.append(pytest.param(5, 600, 40, 25, any_leader, words, base, term, id="5-" + what))
                out.append(pytest.param(5, 600, 40, 4, any_leader, words, base, term, id="5-at-4-percent-" + what))
    return out


@pytest.mark.parametrize("R,G,T,percent,any_leader,words,base,term", _routed_params())
def test_routed_cluster(R, G, T, percent, any_leader, words, base, term):
    nodes, ora, lib, appends, now = routed_cluster_case(R, G, base, term, words=words, any_leader=any_leader, T=T, percent=percent)
    check_cluster_drains(nodes, ora)
    lib.close()


def _replayed(R, base, term, ref_base=None, G=192, n=16):
    """jg_dense_cluster_rounds - the round replayed as a graph, the clock advanced on the device - against the call-by-call
    loop on the device and on the oracle (tests/test_dense_node.py::test_library_driven_rounds_equal_eager_rounds)"""
    from josefine_amd import DenseCluster as LibCluster
    ref_base = base if ref_base is None else ref_base
    shift = (base - ref_base) & M64
    lead = 0 if R == 3 else 2
    appends = np.random.default_rng(R).integers(0, 3, G).astype(np.uint64)
    eager = wide_cluster(DenseCluster, BatchedRaft, G, R, ref_base, term, lead=lead)
    ora = wide_cluster(DenseCluster, oracle_engine, G, R, ref_base, term, lead=lead)
    nodes = wide_cluster_nodes(BatchedRaft, G, R, base, term, lead=lead)
    assert sides(ora.nodes[lead].read("heartbeat_time")) == (ref_base < BOUND, ref_base >= BOUND)
    lib = LibCluster(nodes, lead=lead)
    lib.set_appends(0, appends)
    lib.rounds((base + 100) & M64, 100, n)  # (the first graph of eight rounds carries the clock across 2^32: round 5)
    for _ in range(n):
        eager.round(appends)
        ora.round(appends)
    for r in range(R):
        compare_shifted(nodes[r], eager.nodes[r], shift, f"library-driven vs eager, node {r}")
        compare_shifted(nodes[r], ora.nodes[r], shift, f"library-driven vs oracle, node {r}")
        for fn in ("drain_messages", "drain_faults"):
            got = getattr(nodes[r], fn)()
            want = np.concatenate([rows[r] for rows in ora.rows]) if fn == "drain_messages" else getattr(ora.nodes[r], fn)()
            assert got.tobytes() == want.tobytes(), (r, fn, len(got), len(want))
    L = ora.nodes[lead]
    assert (L.read("role") == capi.ROLE_LEADER).all() and (L.read("term") == np.uint64(term)).all()
    assert int(L.read("head").max()) == int(appends.max()) * n and int(L.read("commit").max()) > 0
    hbt = nodes[lead].read("heartbeat_time")
    # heartbeat_time on both sides of the boundary, read ACROSS the run: every leader beats in the same rounds, so the
    # column never holds both at once - all of it below 2^32 at the start (asserted above), all of it above at the end
    if base == C32:
        assert sides(hbt) == (False, True) and sides(nodes[(lead + 1) % R].read("election_time")) == (False, True)
    assert (hbt - np.uint64(shift) > np.uint64(ref_base + 100 * (n - 2))).all()  # (the last or the last but one round's beat)
    lib.close()


@pytest.mark.parametrize("R,base,term", [pytest.param(3, C32, T32, id="small-3-c32-t32"), pytest.param(3, C63, T63, id="3-c63-t63"),
                                         pytest.param(5, C32, T32, id="5-c32-t32"), pytest.param(5, C63, T63, id="5-c63-t63")])
def test_replayed_closed_loop(R, base, term):
    _replayed(R, base, term)


# ---- 5. the wrap -------------------------------------------------------------------------------------------------------
def test_small_wrap_replayed_closed_loop():
    """the device at now + 2^64 - 450 (its clock wraps inside the first graph), the oracle at now"""
    _replayed(3, CWRAP, T32, ref_base=0)


@pytest.mark.parametrize("R", [3, 5])
def test_small_wrap_dense_halves(R):
    leader_half_case(BatchedRaft, oracle_engine, R, CWRAP, T32, LAYOUT[R], ref_base=0)
    follower_half_case(BatchedRaft, oracle_engine, R, CWRAP, T32, LAYOUT[R], ref_base=0)


# ---- 6. the readers ----------------------------------------------------------------------------------------------------
def test_small_readers_on_the_cluster_end_state():
    """on the routed cluster's end state (R = 3, from 2^63 - 450 and 2^63 - 3): the leadership feed against a host diff of
    the read columns, the census' max_term, point queries of the term and both timers, and export / import with the
    clock shifted back by 2^63 - 450"""
    from test_leader_feed import Feed
    R, G = 3, 192
    nodes, ora, lib, appends, now = routed_cluster_case(R, G, C63, T63, T=12)
    rng = np.random.default_rng(6)
    feeds = [Feed(n) for n in nodes]
    for n, f in enumerate(feeds):
        assert f.check(f"node {n}: first watch") == G  # (Feed.check: the watch == the diff of the columns; the census == numpy's)
    for t in range(3):  # a few more rounds: what changed is reported, nothing else
        lib.round_routed((now + 100 * (t + 1)) & M64, None)
        ora.round(appends)  # (what the library cluster still offers: the trace's last withdrawals and offers)
    for n, f in enumerate(feeds):
        compare_snapshots(nodes[n], ora.nodes[n], f"node {n} before the readers")
        f.check(f"node {n}: second watch")
        c = nodes[n].census()
        assert c["max_term"] == int(nodes[n].read("term").max()) >= T63
        lst = rng.integers(0, G, 3 * G)  # shuffled, with repeats
        rows = nodes[n].lookup(lst)
        for k in ("term", "election_time", "heartbeat_time"):
            assert np.array_equal(rows[k], nodes[n].read(k)[lst]), (n, k)
    # export, then import with the clock shifted back: the copy at now - C63 continues as the source at now
    now += 300
    src, twin = nodes[1], ora.nodes[1]
    copy = BatchedRaft(G, R, seed=6, self_slots=np.full(G, 1, np.uint8), flags=capi.CFG_SEPARATE_COMMIT_KEY)
    copy.import_groups(src.export_groups(), shift_ms=-C63)
    compare_shifted(src, copy, C63, "imported")
    from fuzz import random_batch
    lib.close()
    for s in range(8):
        b = random_batch(rng, twin, 2 * G, budget=np.full(G, 4))
        now += int(rng.integers(50, 400))
        for e, off in ((src, 0), (twin, 0), (copy, -C63)):
            e.submit_columns(**b)
            e.step((now + off) & M64)
        compare_snapshots(src, twin, f"source step {s}")
        compare_shifted(src, copy, C63, f"imported step {s}")
        rows = [e.drain_messages() for e in (src, twin, copy)]
        assert rows[0].tobytes() == rows[1].tobytes() == rows[2].tobytes(), s
        for fn in ("drain_applies", "drain_faults"):
            rows = [getattr(e, fn)() for e in (src, twin, copy)]
            assert rows[0].tobytes() == rows[1].tobytes() == rows[2].tobytes(), (s, fn)


def test_small_watch_reports_a_change_of_the_high_half_once():
    """a follower at term (1 << 32) + 5 with leader L receives a Heartbeat at (2 << 32) + 5 from the same L: only the high
    half of its leadership view changes - reported exactly once"""
    G, R = 64, 3
    dev, ora = BatchedRaft(G, R, seed=3), oracle_engine(G, R, seed=3)
    L = dev.node_ids[1]
    for e in (dev, ora):
        raise_clock([e], C32)
        raise_term([e], (1 << 32) + 5, L, C32)
    rows, total = dev.watch_leaders()
    assert total == G and (rows["term"] == np.uint64((1 << 32) + 5)).all() and (rows["leader_id"] == L).all()
    assert dev.watch_leaders()[1] == 0
    some = np.arange(5, G, 7, dtype=np.uint32)
    for e in (dev, ora):
        raise_term([e], (2 << 32) + 5, L, C32 + 100, some)
    compare_snapshots(dev, ora, "the high half of the term changed")
    peek, total = dev.watch_leaders(peek=True)
    assert total == len(some)
    rows, total = dev.watch_leaders()
    assert total == len(some) and rows.tobytes() == peek.tobytes()
    assert np.array_equal(rows["group"], some) and (rows["term"] == np.uint64((2 << 32) + 5)).all() and (rows["leader_id"] == L).all()
    assert dev.watch_leaders()[1] == 0
    assert dev.census()["max_term"] == (2 << 32) + 5
