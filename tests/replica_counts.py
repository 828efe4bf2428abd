"""Every replica count at the edge of its lag field: the ladder and the node steps of tests/test_replica_counts.py.

A leader's progress heads and its commit index live in ONE 64-bit word of R + 1 fields of 64 / (R + 1) bits (jg_lag_bits,
jg_device.h); the two largest codes of a field are escapes into the wide columns - BEHIND = esc - 1: too far below the
base, ABOVE = esc: above it.  BEHIND is 2 097 150, 65 534, 4 094, 1 022, 510, 254, 126 for R = 2 .. 8.  The engine
instantiates its kernels for every R, and every reader of the word is generic on it; the ladder walks an engine of a few
hundred partitions up to that edge - which a dense tick of up to JG_MAX_DENSE_APPENDS - 1 = 2^20 - 1 appends reaches in one
tick (two at R = 2) - and then over it block by block, and holds EVERYTHING that reads the word to the oracle or to the
numpy statements of the feeds' own tests after every tick.  A driver takes the factories of the engine under test and of
its reference, so the device and the emulated device run the same cases.

Who climbs.  The oracle appends block by block (about 0.55 us per block and partition), so at the two long fields only
some partitions climb and the others append nothing during the climb (they walk the rungs at lags of 1 - 4): at R = 3 the
first 15 partitions of each class (90 x 65 532 blocks), at R = 2 the first partition of classes 1 and 4 (2 x 2 097 148) -
at R = 2 classes 2 and 3 ARE class 1 (the one other member is silent), class 4 differs from it by its stale ack, and
classes 0 and 5 have no silent member whose lag could reach the edge.  From R = 4 on every partition climbs.  `climbers`
asserts the cap of 6 000 000 appended blocks per case from these numbers; nothing here is timed."""
import os

import numpy as np

from josefine_amd import capi
from josefine_amd.traces import elect_all
from parity import compare_snapshots

NO = capi.NO_ACK
MAX_STEP = capi.MAX_DENSE_APPENDS - 1
DRAINS = ("drain_messages", "drain_applies", "drain_faults")
ORACLE_BLOCKS_CAP = 6_000_000
EMULATED = os.environ.get("JG_EMULATED_DEVICE") == "1"  # (the stand-in's wave reductions behind divergent code: tests/host_device.py)
SMALL_TICKS = 3 + 7  # blocks per partition besides the climb: the start's three, four rungs, the forged tick, two rejoin ticks
SILENT_CLASSES = (1, 2, 3, 4)


def behind_of(R):
    return (1 << (64 // (R + 1))) - 2


def own_slots(G, R, layout):
    return {"mixed": (np.arange(G) % R).astype(np.uint8), "uniform": np.full(G, R - 1, np.uint8)}[layout]


def climbers(G, R):
    """(the partitions that climb, as a mask; the classes that are held to the conditions at this R)"""
    g = np.arange(G)
    if R >= 4:
        climb, c, classes = np.ones(G, bool), None, SILENT_CLASSES
    elif R == 3:
        c, classes = 15, SILENT_CLASSES
        climb = g // 6 < c
    else:
        c, classes = 1, (1, 4)
        climb = (g // 6 < c) & np.isin(g % 6, classes)
    blocks = int(climb.sum()) * (behind_of(R) - 2) + G * SMALL_TICKS
    want = G if c is None else c * (6 if R == 3 else len(classes))
    assert int(climb.sum()) == want and blocks <= ORACLE_BLOCKS_CAP, (R, c, int(climb.sum()), blocks)
    return climb, classes


def drain(e):
    return {fn: getattr(e, fn)() for fn in DRAINS}


def same_drains(e, want, what):
    for fn in DRAINS:
        got = getattr(e, fn)()
        assert got.shape == want[fn].shape and got.tobytes() == want[fn].tobytes(), f"{what}: {fn}: {len(got)} rows against {len(want[fn])}"


def ladder(make, make_ref, R, layout, G=357, twin=True):
    """G = 357 = 256 + 64 + 37: one full workgroup, then a partial one whose second wave has 37 lanes.  Every partition is
    led by this engine (own slot g % R, or R - 1 throughout); others[k] is the member k + 1 places behind the own slot.  By
    g % 6:
      0  everybody acknowledges the new head
      1  others[0] is silent
      2  every other member is silent: the quorum is lost, the commit lag grows
      3  others[R / 2 - 1:] are silent: self and R / 2 - 1 others acknowledge - one short of a quorum at even and odd R
      4  others[-1] is silent on appending ticks and acknowledges head - 1 on the quiet tick
      5  steady until the forged tick
    The ticks, each built from the oracle's head column and stepped through step_dense_acks on every engine:
      start    three appends that everybody acknowledges: no progress head and no commit index that escapes later is 0,
               the value a wide column starts with
      climb    steps of min(remaining, 2^20 - 1) appends until the silent lags stand at BEHIND - 2: every big append lands
               while every field is inside its width, so lag space serves it
      rungs    four ticks of one append: lags of BEHIND - 1 (the last that fits), BEHIND, BEHIND + 1, BEHIND + 2; after the
               third the engine is exported into a fresh one with default own slots, which is ticked with the rest from there
      quiet    no append; class 4's stale ack
      forged   one append; class 5's others[0] acknowledges head + 1000 (ABOVE) - at R = 2 that is a quorum, and
               the oracle decides whether it is a fault
      rejoin   two ticks of one append that everybody acknowledges: every BEHIND and wide-commit state comes back through
               the general path into lag space
    After every tick `check` holds the engine to the oracle (every column, every drained row) and every reader of the word
    to its statement: the replication feed at thresholds on both sides of BEHIND and its census, lookup with progress
    heads, the commit feed, and - with `twin` - one poll of a twin engine to the separate calls; at the end the decision
    counters equal the oracle's (on the device: the emulated one only approximates the wave reductions behind them).  Once, after the quiet
    tick, a third engine that was sampled under the time rule right after the election (everybody in sync) is sampled at
    1000, 1400 and 1601 ms with a window of 500 ms: the members that are behind leave at the third sample and not before.
    The conditions at the end of each stage are asserted on the ORACLE's columns: a ladder that no longer reaches its rungs
    fails.  Returns (dev, ora)."""
    from test_commit_feed import Feed as CommitFeed
    from test_lookup_groups import FIELDS
    from test_poll import equal
    from test_replica_clock import Clock
    from test_replica_feed import SEEN_LEADS, census_np, key_of, lags_of, view_of
    B = behind_of(R)
    slots = own_slots(G, R, layout)
    kw = dict(seed=60 + R, flags=capi.CFG_SEPARATE_COMMIT_KEY)
    dev, ora, clk = make(G, R, self_slots=slots, **kw), make_ref(G, R, self_slots=slots, **kw), make(G, R, self_slots=slots, **kw)
    two = make(G, R, self_slots=slots, **kw) if twin else None
    others_ = [x for x in (two, clk) if x is not None]  # device engines that are ticked along and drained
    for e in [ora, dev] + others_:
        elect_all(e)
    compare_snapshots(dev, ora, "election")
    same_drains(dev, drain(ora), "election")
    for e in others_:
        drain(e)
    assert (ora.read("role") == capi.ROLE_LEADER).all() and not ora.read("fault").any()
    clock = Clock(clk, max_behind=500, caught=0, join=0)
    assert clock.sample(900, "elected")[1] == G  # (leaders at genesis: every lag is 0, everybody joins)

    g = np.arange(G)
    cls = g % 6
    climb, classes = climbers(G, R)
    lost = tuple(c for c in classes if c in (2, 3) or R == 2)  # the classes without a quorum
    sl = slots.astype(np.int64)
    other = lambda k: (sl + k + 1) % R  # noqa: E731  (others[k], per partition)
    silent = np.zeros((R, G), bool)     # [member slot][partition]: says nothing on an appending tick
    for k in range(R - 1):
        on = ((cls == 1) & (k == 0)) | (cls == 2) | ((cls == 3) & (k >= R // 2 - 1)) | ((cls == 4) & (k == R - 2))
        silent[other(k), g] = on
    imported = []
    seen = np.zeros(G, np.uint16)
    commits = CommitFeed(dev)
    thresholds = ((B - 1, 0), (B, B - 1), (B + 5, B), (3, 1))

    def tick(n, stale=False, forged=False, everybody=False):
        head = ora.read("head").astype(np.uint64)
        n = np.broadcast_to(np.asarray(n, np.uint64), (G,))
        acks = np.full((R, G), NO, np.uint64)
        for k in range(R - 1):
            r = other(k)
            acks[r, g] = np.where(silent[r, g] & (not everybody), np.uint64(NO), head + n)
        if stale:
            acks[other(R - 2), g] = np.where(cls == 4, head - np.uint64(1), acks[other(R - 2), g])
        if forged:
            acks[other(0), g] = np.where(cls == 5, head + np.uint64(1000), acks[other(0), g])
        acks[sl, g] = n
        for e in [ora, dev] + others_ + imported:
            e.step_dense_acks(acks)

    def check(what, faulted=None):
        want = drain(ora)
        for e in [dev] + imported:
            compare_snapshots(e, ora, what)
            same_drains(e, want, what)
        for e in others_:
            drain(e)
        fault = ora.read("fault")
        assert not fault[~faulted].any() if faulted is not None else not fault.any(), what
        # the replication feed on both sides of BEHIND, against the numpy statement over the columns just compared
        for leave, join in thresholds:
            cur = view_of(dev, seen, leave, join)
            m = key_of(cur) != seen
            rows, total = dev.watch_replicas(leave, join, peek=True)
            assert total == int(m.sum()), (what, leave, join, total, int(m.sum()))
            assert rows.tobytes() == cur[m].tobytes(), (what, leave, join, rows[:4], cur[m][:4])
        answers = dict(leaders=dev.watch_leaders())
        rows, total = answers["replicas"] = dev.watch_replicas(3, 1)
        assert total == int(m.sum()) and rows.tobytes() == cur[m].tobytes(), (what, "delivered")
        seen[rows["group"]] = key_of(rows)
        for limit in (0, B - 1, B, B + 1):
            assert dev.replication_census(limit) == census_np(dev, limit), (what, limit)
        # lookup with progress heads
        rows, match = dev.lookup(progress=True)
        for r in range(R):
            assert np.array_equal(match[:, r], ora.read("match", r)), (what, "lookup: match", r)
        for k in FIELDS:
            assert np.array_equal(rows[k], ora.read(k)), (what, "lookup", k)
        # the commit feed: held to numpy (a peek), then delivered
        peeked = commits.poll(what, peek=True)
        answers["commits"] = dev.watch_commits(backlog=True)
        assert answers["commits"][0].tobytes() == peeked.tobytes() and answers["commits"][1] == len(peeked), what
        commits.advance(peeked)
        if two is not None:  # one poll of the twin against the separate calls (test_poll.both)
            answers["census"], answers["repl_census"] = dev.census(), dev.replication_census(B)
            equal(two.poll(leaders={}, replicas=dict(leave_lag=3, join_lag=1), commits=dict(backlog=True), census=True, repl_census=B), answers, what)

    def having(c, cond):
        """a leading, unfaulted partition of class c meets cond ([G] bool over the oracle's columns)"""
        ok = (ora.read("role") == capi.ROLE_LEADER) & (ora.read("fault") == 0) & (cls == c) & cond
        return bool(ok.any())

    def lags():
        _, head, lag, _ = lags_of(ora, 0, G)
        return lag, head - ora.read("commit").astype(np.uint64)

    tick(3, everybody=True)
    check(f"R={R} start")
    assert (ora.read("commit") == 3).all()
    left = np.where(climb, B - 2, 0).astype(np.uint64)
    t = 0
    while left.any():
        n = np.minimum(left, np.uint64(MAX_STEP))
        tick(n)
        check(f"R={R} climb {t}")
        left, t = left - n, t + 1
    assert t == (2 if R == 2 else 1)
    lag, clag = lags()
    assert all(having(c, lag.max(axis=0) == B - 2) for c in classes) and all(having(c, clag == B - 2) for c in lost)
    for k in range(1, 5):
        tick(1)
        check(f"R={R} rung {k}")
        lag, clag = lags()
        assert all(having(c, lag.max(axis=0) == B - 2 + k) for c in classes), (k, "progress lag")
        assert all(having(c, clag == B - 2 + k) for c in lost), (k, "commit lag")
        if k == 3:
            imp = make(G, R, **kw)
            imp.import_groups(dev.export_groups())
            drain(imp)
            compare_snapshots(imp, dev, "imported")
            imported.append(imp)
    assert all(having(c, lag.max(axis=0) >= B) for c in classes) and all(having(c, clag >= B) for c in lost)
    tick(0, stale=True)
    check(f"R={R} quiet")
    # the time rule: the clocks of the members that are behind start at the first sample and run out at the third
    lag, _ = lags()
    out = np.zeros(G, np.uint8)
    for r in range(R):
        out |= ((lag[r] > 0).astype(np.uint8) << r).astype(np.uint8)
    assert clock.sample(1000, "the clocks start")[1] == 0 and clock.sample(1400, "inside the window")[1] == 0
    rows, total = clock.sample(1601, "the window has passed")
    assert total == int((out != 0).sum()) > 0 and np.array_equal(rows["group"], g[out != 0])
    assert np.array_equal(rows["isr"], ((1 << R) - 1) & ~out[out != 0])
    tick(1, forged=True)
    dead = (cls == 5) if R == 2 else np.zeros(G, bool)
    check(f"R={R} forged", faulted=dead)
    if R > 2:  # (at R = 2 the forged ack is half of the quorum: whether that is a fault is the oracle's to say)
        m0 = np.stack([ora.read("match", r) for r in range(R)])[other(0), g]
        assert having(5, m0 > ora.read("head"))
    for k in range(2):
        tick(1, everybody=True)
        check(f"R={R} rejoin {k}", faulted=dead)
    lag, clag = lags()
    live = ora.read("fault") == 0
    assert live[~dead].all() and (lag[:, live] <= 1).all() and (clag[live] <= 1).all()
    assert (seen[live] == (SEEN_LEADS | ((1 << R) - 1))).all()  # ... and the feed has reported everybody back
    if not EMULATED:
        assert dev.counters()["decisions"] == ora.counters()["decisions"], (dev.counters(), ora.counters())
    return dev, ora


def node_steps(make, make_ref, R, G=300, T=10):
    """tests/test_node_step.py's mixed population (60 % of the partitions led, own slot g % R) under the adversarial row
    traffic of tests/node_step.py through jg_step_node, against the reference's arrival-order step: outbox, every column, the
    three drains, tick by tick.  Both kinds of tick have to occur: with rows for the general path and with rows but none for
    it.  No seed gives the second kind under node_traffic's defaults - at 300 partitions every tick carries 6 - 150 rows for
    the general path, at every R, with or without its noise rows - so the T ticks are followed by three sparse ones (three
    partitions in a hundred get mail, no noise, nothing reordered), of which at least two are of that kind at every R."""
    from node_step import compare_outboxes, node_traffic
    from test_node_step import _same_rows, mixed_pair
    dev, ora, rng = mixed_pair(make, make_ref, G, R, seed=40 + R, election_timeout_ms=(700, 1500), self_slots=(np.arange(G) % R).astype(np.uint8))
    compare_snapshots(dev, ora, "set-up")
    general = plain = 0
    for t in range(T + 3):
        cols = node_traffic(rng, ora, token0=1000 * t, **(dict(p_noise=0.0, quiet=0.97, p_reorder=0.0) if t >= T else {}))
        for e in (dev, ora):
            e.submit_columns(**cols)
        a, b = dev.step_node(100 * (t + 1)), ora.step_node(100 * (t + 1))
        compare_outboxes(a, b, f"R={R} node step {t}")
        compare_snapshots(dev, ora, f"R={R} node step {t}")
        for fn in DRAINS:
            _same_rows(getattr(dev, fn)(), getattr(ora, fn)(), f"R={R} node step {t}: {fn}")
        general += b["rows_general"] > 0
        plain += b["rows_general"] == 0 and b["rows"] > 0
    assert general > 0 and plain > 0, (general, plain)
    if not EMULATED:
        assert dev.counters()["decisions"] == ora.counters()["decisions"], (dev.counters(), ora.counters())
    return dev, ora
