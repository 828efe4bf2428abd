"""Poll under the time rule (ABI v20): jg_poll.clock - jg_engine_poll answers the replicas part as
jg_engine_watch_replicas_timed does, and advances the clocks in its one fused pass.  The poll still defines no value of its
own, so the reference is the separate calls, bit for bit, and the method is tests/test_poll.py's TWINS: two engines of one
seed driven identically, one asked with watch_leaders / watch_replicas_timed / watch_commits / census /
replication_census, the other with one poll(...); everything returned must be byte-equal.  The clocks cannot be read, so
after each stage both twins are PROBED: watch_replicas_timed(peek=True) at several later now_ms - inside the window, just
past it, far past it - whose answers are functions of the stamps and must be equal too.  The small shape is test_poll's
G = 1317: two tiles of the pass, the second with one full row and a 37-lane partial wave.  Cases whose id contains "small"
are small enough for the emulated device (tests/test_poll_timed_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, DenseCluster, capi
from josefine_amd.engine import EngineError
from parity import compare_drains, compare_snapshots
from test_move_groups import drain_all
from test_poll import FEEDS, G_SMALL, LAGS, TILE, both, busy, dtick, equal, poll, ranges, twins
from test_replica_clock import everybody, fall_behind, in_sync
from test_replica_feed import LEADS, U64_MAX, UNDER, dense_tick, elect

pytestmark = pytest.mark.gpu

RULE = dict(max_behind_ms=500, caught_lag=1, join_lag=0)
WINDOW = RULE["max_behind_ms"]


def timed(now, **kw):
    """the replicas options of a poll under the time rule"""
    return dict(RULE, now_ms=now, **kw)


def everything(now, **kw):
    return dict(leaders={}, replicas=timed(now, **kw), commits=dict(backlog=True), census=True, repl_census=1)


def peeks(now):
    return dict(leaders=dict(peek=True), replicas=timed(now, peek=True), commits=dict(peek=True, backlog=True), census=True, repl_census=1)


def calls(e, g0=0, n=None, leaders=None, replicas=None, commits=None, census=False, repl_census=None):
    """the separate calls of the parts named, as the dict poll(...) returns; replicas options that name now_ms are the
    timed watch's"""
    out = {}
    if leaders is not None:
        out["leaders"] = e.watch_leaders(g0, n, leaders.get("limit"), leaders.get("peek", False))
    if replicas is not None and "now_ms" in replicas:
        out["replicas"] = e.watch_replicas_timed(replicas["now_ms"], replicas["max_behind_ms"], replicas.get("caught_lag", 0), replicas.get("join_lag", 0),
                                                 g0, n, replicas.get("limit"), replicas.get("peek", False))
    elif replicas is not None:
        out["replicas"] = e.watch_replicas(replicas["leave_lag"], replicas.get("join_lag"), g0, n, replicas.get("limit"), replicas.get("peek", False))
    if commits is not None:
        out["commits"] = e.watch_commits(g0, n, commits.get("limit"), commits.get("peek", False), commits.get("commits_only", False),
                                         commits.get("backlog", False))
    if census:
        out["census"] = e.census(g0, n)
    if repl_census is not None:
        out["repl_census"] = e.replication_census(repl_census, g0, n)
    return out


HOW = (calls, poll)


def probe(e, now, rule=RULE):
    """what the clocks of e say, without moving them: timed peeks inside the window, at its last millisecond, just past it
    and far past it"""
    out = []
    for later in (now, now + 1, now + rule["max_behind_ms"] // 2, now + rule["max_behind_ms"], now + rule["max_behind_ms"] + 1, now + 10**7):
        rows, total = e.watch_replicas_timed(later, rule["max_behind_ms"], rule["caught_lag"], rule["join_lag"], peek=True)
        out.append((later, total, rows.tobytes()))
    return out


def probes_equal(a, b, now, what, rule=RULE):
    x, y = probe(a, now, rule), probe(b, now, rule)
    for p, q in zip(x, y):
        assert p[:2] == q[:2] and p[2] == q[2], (what, "probe", p[:2], q[:2])
    return x


def restart(es, gs, now):
    """the process of the slots gs restarts on its tree: they stop leading"""
    for e in es:
        e.submit_columns(np.full(len(gs), capi.CMD_RESTART, np.uint8), np.asarray(gs, np.uint32))
        e.step(now)
        drain_all(e)


# ---- 1. every transition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_every_transition(R):
    G = G_SMALL
    a, b = twins(G, R, 40 + R)
    es = (a, b)
    at = np.arange(G)
    esc = (1 << (64 // (R + 1))) - 1
    down = at[at % 7 == 5]     # members that fall silent, in both tiles and the partial wave
    again = at[at % 7 == 2]    # ... a second set, whose clocks run when their slots stop leading
    stop = again[::2]
    shut = np.arange(TILE - 30, TILE + 30)  # closed across the tile border; the first 40 opened again
    far = at % 97 == 0

    def wide():
        dtick(es, np.where(far, esc + 10, 0), lambda k, head, slot: np.where((k == 1) | far, capi.NO_ACK, head).astype(np.uint64))

    def close():
        for e in es:
            e.close_groups(shut)

    def reopen():
        for e in es:
            e.open_groups(shut[:40], 9000)
        elect(es, shut[:40], 9010)

    # (the stage, how far the caller's clock moves before its sample)
    stages = [
        ("fresh", lambda: None, 0),
        ("caught up", lambda: (elect(es, at, 10), in_sync(es)), 100),
        ("members fall silent: their clocks start", lambda: fall_behind(es, G, down), 100),
        ("inside the window", lambda: None, WINDOW // 2),
        ("to its last millisecond", lambda: None, WINDOW - WINDOW // 2),
        ("expiry", lambda: None, 1),
        ("caught up at lag 1: not joined", lambda: dense_tick(es, 1, everybody), 50),
        ("rejoin at join_lag", lambda: dense_tick(es, 0, everybody), 50),
        ("a second set falls silent", lambda: fall_behind(es, G, again), 100),
        ("slots stop leading: their clocks clear", lambda: restart(es, stop, 5000), 100),
        ("... and lead again", lambda: elect(es, stop, 6000), WINDOW + 1),  # (the rest of `again` expires here)
        ("closed", close, 10),
        ("opened", reopen, 10),
        ("a lag on the wide escape", wide, 100),
        ("... expires", lambda: None, WINDOW + 1),
        ("everybody back", lambda: (dense_tick(es, 0, everybody), dense_tick(es, 0, everybody)), 10),
    ]
    seen = {k: 0 for k in FEEDS}
    expired, rejoined = set(), set()
    full = (1 << R) - 1
    now, wide_seen = 1000, False
    for s, (what, stage, dt) in enumerate(stages):
        stage()
        now += dt
        lead = (a.read("role") == capi.ROLE_LEADER) & (a.read("fault") == 0)
        wide_seen = wide_seen or bool(((a.read("head") - a.read("commit"))[lead] >= esc - 1).any())
        how = HOW if s < len(stages) // 2 else HOW[::-1]  # halfway the twins swap
        for g0, n in ranges(G)[1:]:  # (peeks a little ahead of the sample: a clock they stored would be a later one)
            both(a, b, (what, g0, n, "peek"), how, g0=g0, n=n, **peeks(now + 7))
        r = ranges(G)[1 + s % 3]  # a range is delivered, then everything
        part = both(a, b, (what, r), how, g0=r[0], n=r[1], **everything(now))
        got = both(a, b, what, how, **everything(now))
        for k in FEEDS:
            seen[k] += len(part[k][0]) + len(got[k][0])
        rows = np.concatenate([part["replicas"][0], got["replicas"][0]])
        if "expir" in what or "lead again" in what:
            expired |= set((rows["group"][(rows["state"] & UNDER) != 0] // TILE).tolist())
        if "rejoin" in what:
            rejoined |= set((rows["group"][(rows["state"] == LEADS) & (rows["isr"] == full)] // TILE).tolist())
        before = probes_equal(a, b, now, what)
        quiet = both(a, b, (what, "the same now_ms again"), how, **everything(now))
        assert all(quiet[k][1] == 0 for k in FEEDS), what
        assert probes_equal(a, b, now, (what, "again")) == before, what
    # conditions of the test: every feed had rows to compare, and both tiles saw members leave and come back
    assert all(v > 300 for v in seen.values()), seen
    assert expired == {0, 1} and rejoined == {0, 1}, (expired, rejoined)
    assert wide_seen  # (the wide lag was a leading slot's)
    compare_snapshots(a, b, "twins")


def test_small_one_member():
    G = 300
    a, b = twins(G, 1, 3)
    for s, how in enumerate((HOW, HOW[::-1])):
        if s == 0:
            elect((a, b), np.arange(G), 10)
        dtick((a, b), 4, lambda k, head, slot: head)
        got = both(a, b, "R = 1", how, **everything(1000 + s, max_behind_ms=0))
        assert got["commits"][1] == G and got["replicas"][1] == (G if s == 0 else 0)
        probes_equal(a, b, 2000, "R = 1")


# ---- 2. a cap still advances the clocks behind it -----------------------------------------------------------------------------
def test_small_a_cap_still_advances_the_clocks_behind_it():
    G, R = G_SMALL, 3
    a, b = twins(G, R, 50)
    es = (a, b)
    at = np.arange(G)
    elect(es, at, 10)
    in_sync(es)
    both(a, b, "whole sets", HOW, **everything(1000))
    for i, limit in enumerate((0, 1, TILE // 2 - 100)):
        t0 = 10000 * (i + 1)
        down = at[at % 3 == i]  # (the set of the round before catches up meanwhile: it owes its rejoins)
        fall_behind(es, G, down)
        for e in es:
            e.close_groups(np.arange(20 * i, 20 * i + 20))
        r = both(a, b, ("the clocks start behind a limit of", limit), HOW, leaders={}, replicas=timed(t0, limit=limit), commits={})
        assert r["replicas"][1] >= 20 and len(r["replicas"][0]) == min(limit, r["replicas"][1])
        probes_equal(a, b, t0, ("started", limit))
        quiet = both(a, b, ("inside the window", limit), HOW, leaders={}, replicas=timed(t0 + WINDOW, limit=limit), commits={})
        assert quiet["replicas"][1] == r["replicas"][1] - len(r["replicas"][0])
        r = both(a, b, ("expiry", limit), HOW[::-1], leaders={}, replicas=timed(t0 + WINDOW + 1, limit=limit), commits={})
        led = down[down >= 20 * i + 20]
        assert r["replicas"][1] >= len(led) > TILE // 3 and led[-1] > TILE  # (they left on time, in both tiles)
        probes_equal(a, b, t0 + WINDOW + 1, ("expired", limit))
        left = set(r["replicas"][0]["group"].tolist())
        r = both(a, b, ("the rest", limit), HOW, **everything(t0 + WINDOW + 1))
        assert set(led.tolist()) <= left | set(r["replicas"][0]["group"].tolist())
        probes_equal(a, b, t0 + WINDOW + 1, ("delivered", limit))
    compare_snapshots(a, b, "twins")


# ---- 3. every want that includes the replicas, with a clock -------------------------------------------------------------------
def test_small_every_want():
    G, R = G_SMALL, 3
    names = ("leaders", "replicas", "commits", "census", "repl_census")
    a, b = twins(G, R, 5)
    busy((a, b), G, R)
    now = 1000
    wants = [w for w in range(32) if w & capi.POLL_REPLICAS]
    assert len(wants) == 16
    for want in wants:
        now += 300
        full = dict(leaders=dict(limit=700), replicas=timed(now, limit=900), commits=dict(limit=1100, backlog=True), census=True, repl_census=1)
        parts = {k: full[k] for i, k in enumerate(names) if want >> i & 1}
        both(a, b, ("want", want), HOW, **parts)
        probes_equal(a, b, now, ("want", want))
        # a part left out is untouched: a later separate call of it on the polled twin answers what the other's does
        rest = {k: v for k, v in dict(leaders=dict(peek=True), commits=dict(peek=True, backlog=True)).items() if k not in parts}
        equal(calls(a, **rest), calls(b, **rest), ("left out", want))
        dtick((a, b), 1, lambda k, head, slot: np.where((want + slot) % 3 == 0, capi.NO_ACK, head).astype(np.uint64))
    # without JG_POLL_REPLICAS the clock is not looked at: a pointer to one that would be refused is fine, and no clock moves
    before = probes_equal(a, b, now, "before")
    bad = capi.IsrClock(U64_MAX, 0, 1, 4)
    for want in (capi.POLL_CENSUS, capi.POLL_LEADERS | capi.POLL_COMMITS | capi.POLL_REPL_CENSUS):
        p = capi.Poll()
        c, rc = capi.Census(), capi.ReplCensus()
        p.want, p.g0, p.n = want, 0, G
        p.leader_flags = p.commit_flags = capi.WATCH_PEEK
        p.census, p.repl_census, p.clock = C.pointer(c), C.pointer(rc), C.pointer(bad)
        assert b.api.engine_poll(b._h, C.byref(p)) == capi.OK, want
        assert p.replicas_total == 0
    assert probes_equal(a, b, now, "after") == before
    equal(calls(a, **everything(now + 1)), poll(b, **everything(now + 1)), "the rest")


# ---- 4. the two rules, the poll and the watches mixed on one engine ------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_mixing_on_one_engine(R):
    G = G_SMALL
    a, b = twins(G, R, 60 + R)
    busy((a, b), G, R)
    rng = np.random.default_rng(R)
    now, kinds = 1000, set()
    for t in range(10):
        now += int(rng.integers(0, 400))
        rule = timed(now, limit=int(rng.integers(0, G))) if t % 2 else dict(LAGS, limit=int(rng.integers(0, G)))
        kw = dict(g0=(0, 5, 3)[t % 3], n=(None, G - 9, TILE)[t % 3], leaders=dict(limit=int(rng.integers(0, G))), replicas=rule,
                  commits=dict(limit=int(rng.integers(0, G)), backlog=True))
        x = calls(a, **kw)
        if t % 4 < 2:  # the mixed engine: a lag poll or a timed poll ...
            y = poll(b, **kw)
        else:  # ... or a lag watch or a timed watch, and the other two feeds by a poll
            rest = {f: v for f, v in kw.items() if f != "replicas"}
            y = {**poll(b, **rest), **calls(b, g0=kw["g0"], n=kw["n"], replicas=rule)}
            y = {f: y[f] for f in x}
        kinds.add((t % 4 < 2, "now_ms" in rule))
        equal(x, y, ("mixed", t))
        probes_equal(a, b, now, ("mixed", t))
        moved, quiet = rng.random(G) < 0.3, rng.random(G) < 0.3
        dtick((a, b), np.where(moved, 1, 0), lambda k, head, slot: np.where((k == 1) & quiet, capi.NO_ACK, head).astype(np.uint64))
    assert len(kinds) == 4
    equal(calls(a, **everything(now + WINDOW + 1)), poll(b, **everything(now + WINDOW + 1)), "the rest")
    compare_snapshots(a, b, "twins")


# ---- 5. wide values ------------------------------------------------------------------------------------------------------------
def test_small_wide_values():
    """clocks around 2^32 and 2^63 and up to UINT64_MAX - 1, a clock that steps back, windows of 0 and UINT64_MAX, and heads
    above 2^32 whose lags only a caught_lag / join_lag above 2^32 can call caught up"""
    G, R = 300, 3
    hi = (1 << 32) + 5
    a, b = twins(G, R, 2)
    es = (a, b)
    for e in es:
        e.load_chains([([(0, 0), (hi, 0)], hi)] * G, now_ms=10)
    elect(es, np.arange(G), 20)  # (a new leader's progress starts at 0: every member's lag is 2^32 + 5)
    assert (a.read("head") == hi).all()
    T32, T63 = (1 << 32) - 2, (1 << 63) - 3
    walk = [
        ("lag 2^32 + 5 joins under a join_lag of as much", T32, dict(max_behind_ms=10, caught_lag=hi, join_lag=hi), G),
        ("a caught_lag one short of it: the clocks start", T32 + 1, dict(max_behind_ms=10, caught_lag=hi - 1, join_lag=0), 0),
        ("across 2^32, inside the window", T32 + 11, dict(max_behind_ms=10, caught_lag=hi - 1, join_lag=0), 0),
        ("the clock steps back: nobody leaves", 5, dict(max_behind_ms=10, caught_lag=hi - 1, join_lag=0), 0),
        ("a window of UINT64_MAX: never", T63, dict(max_behind_ms=U64_MAX, caught_lag=hi - 1, join_lag=0), 0),
        ("cleared by a caught_lag that wide", T63, dict(max_behind_ms=10, caught_lag=hi, join_lag=5), 0),
        ("a window of 0: in at the sample that sees them behind", T63 + 1, dict(max_behind_ms=0, caught_lag=hi - 1, join_lag=0), 0),
        ("... and at the same clock", T63 + 1, dict(max_behind_ms=0, caught_lag=hi - 1, join_lag=0), 0),
        ("across 2^63 the clock moved: out", T63 + 4, dict(max_behind_ms=0, caught_lag=hi - 1, join_lag=0), G),
        ("a join_lag above 2^32 takes them back", T63 + 5, dict(max_behind_ms=0, caught_lag=hi + 1, join_lag=hi), G),
        ("the last clock there is", U64_MAX - 1, dict(max_behind_ms=0, caught_lag=hi - 1, join_lag=0), 0),
        ("back from there", T63, dict(max_behind_ms=0, caught_lag=hi - 1, join_lag=0), 0),
    ]
    for s, (what, now, rule, want) in enumerate(walk):
        how = HOW if s % 2 else HOW[::-1]
        both(a, b, (what, "peek"), how, replicas=dict(rule, now_ms=now, peek=True), commits=dict(peek=True))
        r = both(a, b, what, how, leaders={}, replicas=dict(rule, now_ms=now), commits={}, repl_census=hi - 1)
        assert r["replicas"][1] == want, (what, r["replicas"][1], want)
        if now < U64_MAX - 10**8:
            probes_equal(a, b, now, what, dict(rule, max_behind_ms=min(rule["max_behind_ms"], 1000)))
    with pytest.raises(EngineError):
        a.poll(replicas=dict(now_ms=U64_MAX, max_behind_ms=10))
    with pytest.raises(TypeError):
        a.poll(replicas=dict(now_ms=5, max_behind_ms=10, leave_lag=3))
    compare_snapshots(a, b, "twins")


# ---- 6. refusals are all-or-nothing ------------------------------------------------------------------------------------------
def test_small_refusals():
    G, R = 300, 3
    a, b = twins(G, R, 4)
    es = (a, b)
    busy(es, G, R, wide_lag=False)  # (the member behind every own slot is two blocks behind)
    for e in es:  # whole sets delivered, then the clocks start: a refused poll that advanced them or the shadow would show
        assert e.watch_replicas_timed(900, WINDOW, 5, 5)[1] == G
        assert e.watch_replicas_timed(1000, WINDOW, 1, 0)[1] == 0
    before = probes_equal(a, b, 1000, "before")
    api, h = a.api, a._h
    dtypes = dict(leaders=capi.LEADER_ROW_DTYPE, replicas=capi.ISR_ROW_DTYPE, commits=capi.COMMIT_ROW_DTYPE)
    poison = {k: np.frombuffer(b"\x5a" * (np.dtype(t).itemsize * G), t).copy() for k, t in dtypes.items()}
    rows = {k: v.copy() for k, v in poison.items()}
    gauges = dict(backlog=capi.CommitBacklog, census=capi.Census, repl_census=capi.ReplCensus)
    out = {k: t() for k, t in gauges.items()}
    for v in out.values():
        C.memset(C.byref(v), 0x5a, C.sizeof(v))
    good = capi.IsrClock(5000, WINDOW, 1, 0)  # (a sample at which every clock has expired)

    def request(**kw):
        p = capi.Poll()
        p.want, p.g0, p.n = 31, 0, G
        p.policy = capi.IsrPolicy(2, 0)
        p.census_lag_limit = 1
        p.clock = C.pointer(good)
        for k in FEEDS:
            setattr(p, k, rows[k].ctypes.data)
            setattr(p, k + "_cap", G)
            setattr(p, k + "_total", 12345)
        p.backlog, p.census, p.repl_census = C.pointer(out["backlog"]), C.pointer(out["census"]), C.pointer(out["repl_census"])
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def refused(what, handle=h, null=False, **kw):
        p = request(**kw)
        assert api.engine_poll(handle, None if null else C.byref(p)) == capi.EINVAL, what
        assert all(rows[k].tobytes() == poison[k].tobytes() for k in FEEDS), what
        assert all(getattr(p, k + "_total") == 12345 for k in FEEDS), what
        assert all(bytes(v) == b"\x5a" * C.sizeof(v) for v in out.values()), what

    def bad_arguments():
        refused("now_ms is UINT64_MAX", clock=C.pointer(capi.IsrClock(U64_MAX, WINDOW, 1, 0)))
        refused("join_lag above caught_lag", clock=C.pointer(capi.IsrClock(5000, WINDOW, 1, 2)))
        refused("... with the replicas alone", want=capi.POLL_REPLICAS, clock=C.pointer(capi.IsrClock(5000, WINDOW, 1, 2)))
        refused("... peeking", replica_flags=capi.WATCH_PEEK, clock=C.pointer(capi.IsrClock(U64_MAX, WINDOW, 1, 0)))
        refused("a null engine", handle=None)
        refused("a null request", null=True)
        refused("want 0", want=0)
        refused("an unknown bit of want", want=32 | 7)
        refused("an unknown leader flag", leader_flags=2)
        refused("an unknown replica flag", replica_flags=capi.WATCH_COMMITS_ONLY)
        refused("an unknown commit flag", commit_flags=4)
        for k in FEEDS:
            refused("null rows with a cap: " + k, **{k: None})
        refused("a null census", census=None)
        refused("a null replication census", repl_census=None)
        refused("a range out of bounds", g0=G - 1, n=2)
        refused("a range that wraps", g0=1, n=0xFFFFFFFF)

    bad_arguments()
    assert probes_equal(a, b, 1000, "after bad arguments") == before
    # kept node steps outstanding: refused, and the kept steps are still viewable afterwards
    for e in es:
        e.step_node_begin(1000, async_=True, keep=True)
        e.step_node_begin(1100, async_=True, keep=True)
    refused("kept node steps")
    refused("kept node steps, peeking", replica_flags=capi.WATCH_PEEK)
    bad_arguments()
    outs = [[e.node_outbox(), e.node_outbox()] for e in es]
    for k in range(2):
        for name, v in outs[0][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][k][name])), (k, name)
    compare_drains(a, b, "kept")
    compare_snapshots(a, b, "kept")
    # neither a clock nor a shadow moved by any of it: the twin was never polled
    probes_equal(a, b, 1000, "after the refusals")
    # a policy that the lag rule refuses is not looked at beside a clock: the next valid poll, which owes everything
    p = request(policy=capi.IsrPolicy(1, 2), clock=C.pointer(capi.IsrClock(1000 + WINDOW + 1, WINDOW, 1, 0)))
    assert api.engine_poll(h, C.byref(p)) == capi.OK
    want = calls(b, **everything(1000 + WINDOW + 1))
    assert (p.leaders_total, p.replicas_total, p.commits_total) == tuple(want[k][1] for k in FEEDS)
    assert p.leaders_total == G and p.commits_total == G and p.replicas_total > 0
    for k in FEEDS:
        assert rows[k][:want[k][1]].tobytes() == want[k][0].tobytes(), k
    r = both(a, b, "delivered", HOW, **everything(1000 + WINDOW + 1))
    assert all(r[k][1] == 0 for k in FEEDS)


# ---- 7. shards -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [pytest.param(2, id="small-2-shards"), pytest.param(3, id="small-3-shards")])
def test_shards(D):
    G, R = 1003, 3  # ragged: the shards differ in size
    s = BatchedRaft(G, R, seed=4, device_ids=[0] * D)
    one = BatchedRaft(G, R, seed=4)
    first, second, last = s.shard(0).G, s.shard(1).group_lo + s.shard(1).G, s.shard(D - 1).group_lo
    how = (poll, calls)  # the sharded handle polls, the single-device twin is asked with the separate calls
    r = both(s, one, "fresh", how, **everything(5))
    assert r["leaders"][1] == G and r["replicas"][1] == 0
    for e in (s, one):
        elect((e,), np.arange(G), 10)
        in_sync((e,))
    both(s, one, "a range across the shard border", how, g0=first - 5, n=11, **peeks(1000))
    r = both(s, one, "whole sets", how, **everything(1000))
    assert r["replicas"][1] == G
    down = np.concatenate([np.arange(3, first, 50), np.arange(last + 1, G, 9)])
    shut = np.arange(0, 40)
    for e in (s, one):
        fall_behind((e,), G, down)
        e.close_groups(shut)
    # a timed peek advances no shard's clocks: a later probe would see them run
    both(s, one, "a timed peek", how, **peeks(1500))
    both(s, one, "... moved nothing: this far past it nobody has left", how, replicas=timed(10**6, peek=True))
    assert calls(s, replicas=timed(10**6, peek=True))["replicas"][1] == len(shut)
    # the replicas' cap ends inside shard 0, the commits' inside shard 1, the leaders' not at all - and the clocks of the last
    # shard start all the same
    r = both(s, one, "caps that end in different shards", how, leaders={}, replicas=timed(2000, limit=15),
             commits=dict(limit=first + (second - first) // 2, backlog=True), census=True, repl_census=0)
    assert r["replicas"][1] == 40 and r["replicas"][0]["group"].tolist() == list(range(15)) and 15 < first
    assert first <= r["commits"][0]["group"][-1] < second - 1
    probes_equal(s, one, 2000, "started behind the cap")
    r = both(s, one, "inside the window", how, leaders={}, replicas=timed(2000 + WINDOW, limit=5), commits=dict(limit=3))
    assert r["replicas"][1] == 25
    # ... followed by expiry in the last shard, on time
    r = both(s, one, "expiry", how, **everything(2000 + WINDOW + 1))
    led = down[down >= 40]
    assert r["replicas"][1] == 20 + len(led) and set(led.tolist()) <= set(r["replicas"][0]["group"].tolist()) and r["replicas"][0]["group"][-1] >= last
    assert int((down >= last).sum()) > 5
    assert all(v[1] == 0 for k, v in both(one, s, "quiet", how[::-1], **everything(2000 + WINDOW + 1)).items() if k in FEEDS)
    both(s, one, "a cap of 0", how, leaders=dict(limit=1), replicas=timed(9000, limit=0), commits=dict(commits_only=True, limit=second))
    for e in (s, one):
        in_sync((e,))
    assert both(s, one, "back", how, **everything(9000))["replicas"][1] == len(led)
    probes_equal(s, one, 9000, "the end")
    compare_snapshots(s, one, "shards")


# ---- 8. launches ------------------------------------------------------------------------------------------------------------
def test_small_launches():
    G, R = G_SMALL, 3
    a, b = twins(G, R, 8)
    busy((a, b), G, R, wide_lag=False)
    for now, what in ((1000, "everything moved"), (1001, "quiet")):
        feeds = dict(leaders={}, replicas=timed(now), commits=dict(backlog=True))
        la, lb = a.counters()["launches"], b.counters()["launches"]
        both(a, b, what, HOW, **feeds)
        la, lb = a.counters()["launches"] - la, b.counters()["launches"] - lb
        # one count pass and one scan instead of three of each: count, scan, backlog sum and the three write passes
        assert (la, lb) == (10, 6), (what, la, lb)


# ---- 9. the stride (the device only) ----------------------------------------------------------------------------------------
def test_the_stride():
    from josefine_amd.traces import elect_all
    G, R = 1024 * 1024 + 1024 + 37, 3  # more tiles than the grid cap of the fused pass: workgroups take a second tile
    rng = np.random.default_rng(6)
    slots = (np.arange(G) % R).astype(np.uint8)
    a, b = BatchedRaft(G, R, seed=5, self_slots=slots), BatchedRaft(G, R, seed=5, self_slots=slots)
    for e in (a, b):
        elect_all(e, 10)
        drain_all(e)
    dtick((a, b), 3, lambda k, head, slot: head)
    dtick((a, b), 0, lambda k, head, slot: head)
    r = both(a, b, "everything moved", HOW, **everything(1000))
    assert r["leaders"][1] == G and r["replicas"][1] == G and r["commits"][1] == G
    down = rng.random(G) < 0.01
    quiet = lambda k, head, slot: np.where((k == 1) & down, capi.NO_ACK, head).astype(np.uint64)  # noqa: E731
    dtick((a, b), 2, quiet)
    dtick((a, b), 0, quiet)
    r = both(a, b, "the clocks of one percent start", HOW, **everything(2000))
    assert r["replicas"][1] == 0 and r["commits"][1] == G
    r = both(a, b, "... and expire", HOW, leaders={}, replicas=timed(2000 + WINDOW + 1, limit=4000), commits=dict(backlog=True))
    assert r["replicas"][1] == int(down.sum()) and len(r["replicas"][0]) == 4000 and r["replicas"][0]["group"][-1] < G // 2
    r = both(a, b, "the rest of them", HOW[::-1], **everything(2000 + WINDOW + 1))
    assert r["replicas"][1] == int(down.sum()) - 4000 and r["replicas"][0]["group"][-1] > G - TILE


# ---- 10. a node of a dense cluster, between rounds ----------------------------------------------------------------------------
def test_small_cluster_nodes():
    from test_any_leader import spread_leaders
    G, R = 120, 3
    libs = []
    for _ in range(2):
        nodes = [BatchedRaft(G, R, seed=5 + r, self_slots=np.full(G, r, np.uint8), flags=capi.CFG_SEPARATE_COMMIT_KEY) for r in range(R)]
        spread_leaders(nodes, G, R)
        lib = DenseCluster(nodes, lead=None)
        lib.set_appends(per_group=(np.arange(G) % 4).astype(np.uint64))
        libs.append((lib, nodes))
    now, rows = 100, 0
    for p in range(3):
        for lib, _ in libs:
            lib.rounds(now, 100, 8)
        now += 800
        for k in range(R):
            x, y = libs[0][1][k], libs[1][1][k]
            r = both(x, y, f"poll {p} node {k}", HOW if (p + k) % 2 else HOW[::-1], **everything(now, caught_lag=0))
            rows += r["commits"][1] + r["replicas"][1]
            assert r["census"]["leaders"] > 0 and r["census"]["followers"] > 0
            probes_equal(x, y, now, f"poll {p} node {k}", dict(RULE, caught_lag=0))
    assert rows > G
    for lib, _ in libs:
        lib.close()
