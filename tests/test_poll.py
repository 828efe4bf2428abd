"""One poll per tick (ABI v18): jg_engine_poll answers the three change feeds and the two censuses in one call - one
settle, one fused count pass, one synchronisation.  It defines no value of its own, so the reference is the separate calls,
bit for bit.  The method throughout is TWINS: two engines of one seed and config driven identically, one asked with the
separate calls (watch_leaders, watch_replicas, watch_commits, census, replication_census), the other with poll(...);
everything returned must be equal byte for byte, and where a case swaps which twin uses which, the shadows are shown to
have advanced identically.  The pass works in tiles of 1024 slots, rows of 256 and waves of 64: the small shape is
G = 1317 - two tiles, the second with one full row and a 37-lane partial wave.  Cases whose id contains "small" are small
enough for the emulated device (tests/test_poll_emulated.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, DenseCluster, capi, move_groups
from josefine_amd.engine import EngineError
from fuzz import random_batch
from parity import compare_drains, compare_snapshots
from test_commit_feed import same
from test_lookup_groups import tick, world
from test_move_groups import drain_all
from test_replica_feed import elect
from test_vacant_groups import DRAINS, fresh

pytestmark = pytest.mark.gpu

TILE = 256 * 4  # slots per tile of the fused pass (jg_poll.h JG_POLL_TILE)
G_SMALL = TILE + 256 + 37
LAGS = dict(leave_lag=2, join_lag=0)
FEEDS = ("leaders", "replicas", "commits")
EVERYTHING = dict(leaders={}, replicas=dict(LAGS), commits=dict(backlog=True), census=True, repl_census=1)


def ranges(G):
    return ((0, G), (5, G - 9), (3, TILE), (G - 1, 1), (7, 0))


def calls(e, g0=0, n=None, leaders=None, replicas=None, commits=None, census=False, repl_census=None):
    """the separate calls of the parts named, as the dict poll(...) returns"""
    out = {}
    if leaders is not None:
        out["leaders"] = e.watch_leaders(g0, n, leaders.get("limit"), leaders.get("peek", False))
    if replicas is not None:
        out["replicas"] = e.watch_replicas(replicas["leave_lag"], replicas.get("join_lag"), g0, n, replicas.get("limit"), replicas.get("peek", False))
    if commits is not None:
        out["commits"] = e.watch_commits(g0, n, commits.get("limit"), commits.get("peek", False), commits.get("commits_only", False),
                                         commits.get("backlog", False))
    if census:
        out["census"] = e.census(g0, n)
    if repl_census is not None:
        out["repl_census"] = e.replication_census(repl_census, g0, n)
    return out


def poll(e, g0=0, n=None, **parts):
    return e.poll(g0=g0, n=n, **parts)


def equal(x, y, what=""):
    assert list(x) == list(y), (what, list(x), list(y))
    for k in x:
        if k in FEEDS:
            assert x[k][1:] == y[k][1:], (what, k, x[k][1:], y[k][1:])
            same(x[k][0], y[k][0], (what, k))
        else:
            assert x[k] == y[k], (what, k, x[k], y[k])


def both(a, b, what="", how=(calls, poll), **kw):
    """a asked one way, b the other: equal.  Returns a's answer."""
    x, y = how[0](a, **kw), how[1](b, **kw)
    equal(x, y, what)
    return x


def twins(G, R, seed, **kw):
    slots = np.random.default_rng(seed).integers(0, R, G).astype(np.uint8)
    return fresh(G, R, seed, slots, **kw)[0], fresh(G, R, seed, slots, **kw)[0]


def dtick(es, appends, ack):
    """one dense tick on every engine alike (test_lookup_groups.tick): every healthy leader appends appends[g] blocks;
    ack(k, head, slot)[g]: what the member k behind the own slot acknowledges (NO_ACK: silent)"""
    for e in es:
        tick(e, appends, lambda k: ack(k, e.read("head").astype(np.uint64), e.read("self_slot").astype(np.int64)))


def busy(es, G, R, wide_lag=True):
    """every slot leads, has committed three blocks and appended two more that the member behind the own slot has not
    acknowledged; a few slots have a lag field on the wide escape"""
    at = np.arange(G)
    elect(es, at, 10)
    dtick(es, 3, lambda k, head, slot: head)
    dtick(es, 2, lambda k, head, slot: np.where(k == 1, capi.NO_ACK, head).astype(np.uint64))
    if wide_lag and R > 1:
        esc = (1 << (64 // (R + 1))) - 1
        dtick(es, np.where(at % 97 == 0, esc + 10, 0), lambda k, head, slot: np.where((k == 1) | (at % 97 == 0), capi.NO_ACK, head).astype(np.uint64))


# ---- 1. every kind of slot and transition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_every_kind_of_slot_and_transition(R):
    G = G_SMALL
    rng = np.random.default_rng(R)
    a, b = twins(G, R, 11 + R)
    es = (a, b)
    at = np.arange(G)
    zoo = world(R)  # (test_lookup_groups: 300 slots in every state the decodes distinguish; only read here)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    esc = (1 << (64 // (R + 1))) - 1

    def rows(now):
        batch = random_batch(rng, b, 2 * G, foreign_voters=True, budget=budget)
        for e in es:
            e.submit_columns(**batch)
            e.step(now)
            drain_all(e)

    def zoo_in():
        for e in es:
            e.close_groups(np.arange(900, 1200))
            move_groups(zoo.e, e, 0, 300, dst_g0=900)

    def shut():
        for e in es:
            e.close_groups(np.arange(40, 90))
            e.close_groups(np.arange(1300, G))

    def reopen():
        for e in es:
            e.open_groups(np.arange(40, 70), 9000)
            e.load_chains([([(0, 0)] + [(i, i - 1) for i in range(1, k + 4)], k + 2) for k in range(8)], now_ms=9100, g0=1300)

    stages = [
        ("fresh", lambda: None),
        ("elected", lambda: elect(es, at[at % 3 != 1], 10)),
        ("appended", lambda: dtick(es, 3, lambda k, head, slot: head)),
        ("ragged acks", lambda: dtick(es, 2, lambda k, head, slot: np.where((k == 1) & (at % 4 == 0), capi.NO_ACK, head).astype(np.uint64))),
        ("general rows", lambda: rows(700)),
        ("a wide lag", lambda: dtick(es, np.where(at % 50 == 0, esc + 10, 1), lambda k, head, slot: np.where(at % 50 == 0, capi.NO_ACK, head).astype(np.uint64))),
        ("the zoo imported across the tile border", zoo_in),
        ("general rows again", lambda: rows(1500)),
        ("closed", shut),
        ("opened and loaded", reopen),
        ("caught up", lambda: dtick(es, 0, lambda k, head, slot: head)),
        ("a second election", lambda: elect(es, np.arange(40, 70), 20000)),  # (the slots opened a moment ago)
        ("the last tick", lambda: dtick(es, 1, lambda k, head, slot: head)),
    ]
    seen = {k: 0 for k in FEEDS}
    wide = False
    for s, (what, stage) in enumerate(stages):
        stage()
        lead = (a.read("role") == capi.ROLE_LEADER) & (a.read("fault") == 0)
        wide = wide or bool(((a.read("head") - a.read("commit"))[lead] >= esc - 1).any())
        how = (calls, poll) if s < len(stages) // 2 else (poll, calls)  # halfway the twins swap
        for g0, n in ranges(G)[1:]:
            both(a, b, (what, g0, n, "peek"), how, g0=g0, n=n, leaders=dict(peek=True), replicas=dict(LAGS, peek=True),
                 commits=dict(peek=True, backlog=True), census=True, repl_census=1)
        r = ranges(G)[1 + s % 3]  # a range is delivered, then everything
        both(a, b, (what, r), how, g0=r[0], n=r[1], **EVERYTHING)
        got = both(a, b, what, how, **EVERYTHING)
        for k in FEEDS:
            seen[k] += len(got[k][0])
        quiet = both(a, b, (what, "quiet"), how, **EVERYTHING)
        assert all(quiet[k][1] == 0 for k in FEEDS), what
    # conditions of the test: the zoo arrived, and every feed had rows of every kind to compare
    c = a.census()
    assert c["vacant"] and c["faulted_reference"] and c["candidates"] and c["leaders"] and c["followers"]
    assert lead[900:1200].any() and wide
    assert all(v > 300 for v in seen.values()), seen
    compare_snapshots(a, b, "twins")


def test_small_one_replica():
    G = 300
    a, b = twins(G, 1, 3)
    for s, how in enumerate(((calls, poll), (poll, calls))):
        if s == 0:
            elect((a, b), np.arange(G), 10)
        dtick((a, b), 4, lambda k, head, slot: head)
        got = both(a, b, "R = 1", how, **EVERYTHING)
        assert got["commits"][1] == G and got["replicas"][1] == (G if s == 0 else 0)


# ---- 2. all 31 values of want -----------------------------------------------------------------------------------------------
def test_small_every_want():
    G, R = G_SMALL, 3
    names = ("leaders", "replicas", "commits", "census", "repl_census")
    full = dict(leaders=dict(limit=700), replicas=dict(LAGS, limit=900), commits=dict(limit=1100, backlog=True), census=True, repl_census=1)
    a, b = twins(G, R, 5)
    busy((a, b), G, R)
    untouched = dict(leaders=dict(peek=True), replicas=dict(LAGS, peek=True), commits=dict(peek=True, backlog=True))
    for want in range(1, 32):
        parts = {k: full[k] for i, k in enumerate(names) if want >> i & 1}
        both(a, b, ("want", want), **parts)
        # a part left out is untouched: a later separate call of it on the polled twin answers what the other's does
        rest = {k: v for k, v in untouched.items() if k not in parts}
        equal(calls(a, **rest), calls(b, **rest), ("left out", want))
        dtick((a, b), 1, lambda k, head, slot: np.where((want + slot) % 3 == 0, capi.NO_ACK, head).astype(np.uint64))
        if want % 8 == 0:
            for e in (a, b):
                e.close_groups(np.arange(want * 10, want * 10 + 7))
    equal(calls(a, **EVERYTHING), calls(b, **EVERYTHING), "the rest")
    # a feed never asked for has no shadow: the engine that polls only censuses pays for none (its first watch starts at zero)
    c, d = twins(300, R, 6)
    busy((c, d), 300, R, wide_lag=False)
    equal(poll(c, census=True, repl_census=0), calls(d, census=True, repl_census=0), "censuses alone")
    both(c, d, "first watches", **EVERYTHING)


# ---- 3. caps and peeks per feed, independently --------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_caps_and_peeks_per_feed(R):
    G = G_SMALL
    a, b = twins(G, R, 20 + R)
    busy((a, b), G, R)
    for e in (a, b):
        e.close_groups(np.arange(1000, 1050))  # (nothing to report from a slot that never led: the totals differ per feed)
        e.open_groups(np.arange(1000, 1020), 500)
    total = {k: v[1] for k, v in calls(a, leaders=dict(peek=True, limit=0), replicas=dict(LAGS, peek=True, limit=0), commits=dict(peek=True, limit=0)).items()}
    assert len(set(total.values())) > 1 and min(total.values()) > TILE, total
    caps = lambda t: (0, 1, t - 1, t + 3)  # noqa: E731
    combos = [p for p in itertools.product(range(4), repeat=3) if len(set(p)) > 1]
    for i, (x, y, z) in enumerate(combos[::5]):  # caps that differ between the feeds within one call; a peek advances nothing
        peek = FEEDS[i % 3]
        co = dict(commits_only=bool(i & 1), backlog=bool(i & 2))
        both(a, b, ("caps", x, y, z, peek, co), g0=(0, 5)[i % 2], n=(None, G - 9)[i % 2],
             leaders=dict(limit=caps(total["leaders"])[x], peek=True), replicas=dict(LAGS, limit=caps(total["replicas"])[y], peek=True),
             commits=dict(limit=caps(total["commits"])[z], peek=True, **co))
    got = {k: [] for k in FEEDS}
    left = dict(total)
    for i in range(12):  # delivery: peek on one feed only, the others advance; the remainder follows
        peek = FEEDS[i % 3] if i < 6 else None
        cap = {k: (1, left[k] // 3 + 1, 0, left[k] - 1, left[k] + 3, 2)[(i + j) % 6] for j, k in enumerate(FEEDS)}
        co = dict(commits_only=i % 4 == 1, backlog=i % 4 < 2)
        r = both(a, b, ("delivery", i, cap, peek), leaders=dict(limit=cap["leaders"], peek=peek == "leaders"),
                 replicas=dict(LAGS, limit=cap["replicas"], peek=peek == "replicas"), commits=dict(limit=cap["commits"], peek=peek == "commits", **co))
        for k in FEEDS:
            if not (k == "commits" and co["commits_only"]):
                assert r[k][1] == left[k], (i, k, r[k][1], left[k])
            assert len(r[k][0]) == min(max(cap[k], 0), r[k][1])
            if k != peek:
                got[k].append(r[k][0])
                left[k] -= len(r[k][0])
    r = both(a, b, "the remainder", **EVERYTHING)
    for k in FEEDS:
        rows = np.concatenate(got[k] + [r[k][0]])
        assert len(rows) == total[k] and (np.diff(rows["group"].astype(np.int64)) > 0).all(), k  # nothing lost, nothing repeated
    assert all(v[1] == 0 for k, v in both(a, b, "quiet", **EVERYTHING).items() if k in FEEDS)


# ---- 4. values that differ only above bit 32 --------------------------------------------------------------------------------
def test_small_wide_values():
    G, R = 8, 3
    a, b = twins(G, R, 1)
    es = (a, b)
    run = [(0, 0)] + [(i, i - 1) for i in range(1, 6)]
    hi = (1 << 32) + 5

    def step(now, *cmds):
        for e in es:
            for g in (0, 1):
                for c in cmds:
                    e.submit(g, c)
            e.step(now)
            drain_all(e)

    def look(what, how, **counts):
        r = both(a, b, what, how, **EVERYTHING)
        for k, want in counts.items():
            assert r[k][1] == want, (what, k, r[k][1], want)
            assert both(a, b, what + ": delivered", how, **EVERYTHING)[k][1] == 0
        return r

    for e in es:
        e.load_chains([(run, 5)] * 4, now_ms=10)
    look("commit 5, head 5", (calls, poll), commits=4)
    # a term of 2^32 + 7, then 2 * 2^32 + 7: the low halves are equal
    step(20, Command.Heartbeat((1 << 32) + 7, 5, 2))
    r = look("term 2^32 + 7", (poll, calls), leaders=2, commits=0)
    assert (r["leaders"][0]["term"] == (1 << 32) + 7).all()
    step(30, Command.Heartbeat((2 << 32) + 7, 5, 2))
    r = look("term 2 * 2^32 + 7", (calls, poll), leaders=2, commits=0)
    assert (r["leaders"][0]["term"] == (2 << 32) + 7).all()
    # the head alone moves, by 2^32 exactly, then the commit alone, then both back down
    step(40, Command.AppendEntries((2 << 32) + 7, 2, [(hi, 5)]))
    assert a.read("head")[:2].tolist() == [hi, hi] and a.read("commit")[:2].tolist() == [5, 5]
    both(a, b, "commits only: the head is not looked at", (poll, calls), leaders={}, commits=dict(commits_only=True, backlog=True))
    r = look("head 2^32 + 5", (poll, calls), leaders=0, commits=2)
    assert (r["commits"][0]["head_from"] == 5).all() and (r["commits"][0]["state"] == capi.CMT_APPENDED).all()
    step(50, Command.Heartbeat((2 << 32) + 7, hi, 2))
    r = look("commit 2^32 + 5", (calls, poll), leaders=0, commits=2)
    assert (r["commits"][0]["commit_from"] == 5).all() and (r["commits"][0]["state"] == capi.CMT_COMMITTED).all()
    for e in es:
        e.load_chains([(run, 5)], now_ms=60)
    r = look("back at 5", (poll, calls), commits=1)
    assert (r["commits"][0]["state"] == capi.CMT_REWOUND).all()
    # ids near 2^56, and a block on top, committed
    top = 1 << 56
    big = [(0, 0), (1, 0), (top - 1, 1), (top, top - 1)]
    for e in es:
        e.load_chains([(big, top), (big, 1)], now_ms=70, g0=4)
    look("ids near 2^56", (calls, poll), commits=2)
    for e in es:
        e.submit(4, Command.AppendEntries(1, 2, [(top + 1, top)]))
        e.submit(4, Command.Heartbeat(1, top + 1, 2))
        e.step(2000)
        drain_all(e)
    r = look("a block on top, committed", (poll, calls), commits=1)
    assert r["commits"][0]["commit"].tolist() == [top + 1] and r["commits"][0]["state"].tolist() == [capi.CMT_COMMITTED | capi.CMT_APPENDED]
    compare_snapshots(a, b, "twins")


# ---- 5. refusals are all-or-nothing ------------------------------------------------------------------------------------------
def test_small_refusals():
    G, R = 300, 3
    a, b = twins(G, R, 4)
    busy((a, b), G, R, wide_lag=False)
    api, h = a.api, a._h
    dtypes = dict(leaders=capi.LEADER_ROW_DTYPE, replicas=capi.ISR_ROW_DTYPE, commits=capi.COMMIT_ROW_DTYPE)
    poison = {k: np.frombuffer(b"\x5a" * (np.dtype(t).itemsize * G), t).copy() for k, t in dtypes.items()}
    rows = {k: v.copy() for k, v in poison.items()}
    gauges = dict(backlog=capi.CommitBacklog, census=capi.Census, repl_census=capi.ReplCensus)
    out = {k: t() for k, t in gauges.items()}
    for v in out.values():
        C.memset(C.byref(v), 0x5a, C.sizeof(v))

    def request(**kw):
        p = capi.Poll()
        p.want, p.g0, p.n = 31, 0, G
        p.policy = capi.IsrPolicy(2, 0)
        p.census_lag_limit = 1
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
        refused("a null engine", handle=None)
        refused("a null request", null=True)
        refused("want 0", want=0)
        refused("an unknown bit of want", want=32 | 7)
        refused("an unknown bit of want alone", want=1 << 31)
        refused("an unknown leader flag", leader_flags=2)
        refused("an unknown replica flag", replica_flags=capi.WATCH_COMMITS_ONLY)
        refused("an unknown commit flag", commit_flags=4)
        refused("join_lag above leave_lag", policy=capi.IsrPolicy(1, 2))
        for k in FEEDS:
            refused("null rows with a cap: " + k, **{k: None})
        refused("a null census", census=None)
        refused("a null replication census", repl_census=None)
        refused("a range out of bounds", g0=G - 1, n=2)
        refused("a range that wraps", g0=1, n=0xFFFFFFFF)

    bad_arguments()
    # what is wrong with a part NOT wanted is not looked at
    p = request(want=capi.POLL_CENSUS, leader_flags=99, policy=capi.IsrPolicy(1, 2), leaders=None, commits=None, repl_census=None)
    assert api.engine_poll(h, C.byref(p)) == capi.OK and out["census"].leaders == G
    C.memset(C.byref(out["census"]), 0x5a, C.sizeof(out["census"]))
    with pytest.raises(EngineError):
        a.poll(leaders={}, g0=G, n=1)
    with pytest.raises(EngineError):
        a.poll()
    # kept node steps outstanding: refused, and the kept steps are still viewable afterwards
    for e in (a, b):
        e.step_node_begin(1000, async_=True, keep=True)
        e.step_node_begin(1100, async_=True, keep=True)
    refused("kept node steps")
    bad_arguments()
    outs = [[e.node_outbox(), e.node_outbox()] for e in (a, b)]
    for k in range(2):
        for name, v in outs[0][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][k][name])), (k, name)
    compare_drains(a, b, "kept")
    compare_snapshots(a, b, "kept")
    # no shadow moved by any of it: the next valid poll equals the twin's separate calls, and owes everything
    r = both(b, a, "after the refusals", **EVERYTHING)
    assert r["leaders"][1] == G and r["commits"][1] == G
    # n == 0: OK, totals 0, zeroed gauges, rows untouched
    p = request(g0=G, n=0)
    assert api.engine_poll(h, C.byref(p)) == capi.OK
    assert all(getattr(p, k + "_total") == 0 for k in FEEDS) and all(bytes(v) == bytes(C.sizeof(v)) for v in out.values())
    assert all(rows[k].tobytes() == poison[k].tobytes() for k in FEEDS)


# ---- 6. mixing: the poll and the separate calls share the shadows -----------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_mixing_on_one_engine(R):
    G = G_SMALL
    a, b = twins(G, R, 30 + R)
    busy((a, b), G, R)
    rng = np.random.default_rng(R)
    for t in range(10):
        kw = dict(g0=(0, 5, 3)[t % 3], n=(None, G - 9, TILE)[t % 3], leaders=dict(limit=int(rng.integers(0, G))),
                  replicas=dict(LAGS, limit=int(rng.integers(0, G))), commits=dict(limit=int(rng.integers(0, G)), backlog=True, commits_only=t % 5 == 4))
        x = calls(a, **kw)
        if t % 2:  # the mixed engine: a poll ...
            y = poll(b, **kw)
        else:  # ... or one feed by its own call and the other two by a poll, in either order
            k = FEEDS[(t // 2) % 3]
            rest = {f: v for f, v in kw.items() if f != k}
            if t % 4:
                y = {**calls(b, g0=kw["g0"], n=kw["n"], **{k: kw[k]}), **poll(b, **rest)}
            else:
                y = {**poll(b, **rest), **calls(b, g0=kw["g0"], n=kw["n"], **{k: kw[k]})}
            y = {f: y[f] for f in x}
        equal(x, y, ("mixed", t))
        moved, silent = rng.random(G) < 0.3, rng.random(G) < 0.3
        dtick((a, b), np.where(moved, 1, 0), lambda k, head, slot: np.where((k == 1) & silent, capi.NO_ACK, head).astype(np.uint64))
    equal(calls(a, **EVERYTHING), poll(b, **EVERYTHING), "the rest")
    compare_snapshots(a, b, "twins")


# ---- 7. polling changes nothing -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_fuzz_and_polling_changes_nothing(R):
    G = 96
    rng = np.random.default_rng(11 + R)
    a, b = twins(G, R, 5)  # a is polled, b never is
    c = twins(G, R, 5)[0]  # ... and c is asked with the separate calls
    es = (a, b, c)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    elect(es, np.arange(0, G, 2), 10)

    def look(what):
        equal(poll(a, g0=10, n=50, leaders=dict(limit=3, peek=True), commits=dict(limit=2), census=True),
              calls(c, g0=10, n=50, leaders=dict(limit=3, peek=True), commits=dict(limit=2), census=True), what)
        equal(poll(a, **EVERYTHING), calls(c, **EVERYTHING), what)

    now = 10
    for s in range(12):
        batch = random_batch(rng, b, 3 * G, foreign_voters=True, budget=budget)
        now += int(rng.integers(0, 300))
        for e in es:
            e.submit_columns(**batch)
            e.step(now)
        look(f"step {s}")
        for fn in DRAINS:
            x = getattr(b, fn)().tobytes()
            assert getattr(a, fn)().tobytes() == x and getattr(c, fn)().tobytes() == x, (s, fn)
        compare_snapshots(a, b, f"step {s}")
    for t in range(6):  # node steps, JG_NODE_ASYNC: the poll settles the step, once
        now += int(rng.integers(100, 400))
        batch = random_batch(rng, b, G, foreign_voters=True, budget=budget)
        outs = []
        for e in es:
            e.submit_columns(**batch)
            e.step_node_begin(now, async_=True)
            if e is a:
                assert a.poll(census=True, repl_census=1, leaders=dict(peek=True)).keys() == {"leaders", "census", "repl_census"}
            outs.append(e.node_outbox())
        for name, x in outs[1].items():
            assert np.array_equal(np.asarray(x), np.asarray(outs[0][name])) and np.array_equal(np.asarray(x), np.asarray(outs[2][name])), (t, name)
        look(f"node {t}")
        compare_drains(a, b, f"node {t}")
        compare_snapshots(a, b, f"node {t}")
        drain_all(c)


# ---- 8. shards -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [pytest.param(2, id="small-2-shards"), pytest.param(3, id="small-3-shards")])
def test_shards(D):
    G, R = 1003, 3  # ragged: the shards differ in size
    s = BatchedRaft(G, R, seed=4, device_ids=[0] * D)
    one = BatchedRaft(G, R, seed=4)
    first, second = s.shard(0).G, s.shard(1).group_lo + s.shard(1).G
    how = (poll, calls)  # the sharded handle polls, the single-device twin is asked with the separate calls
    r = both(s, one, "fresh", how, **EVERYTHING)
    assert r["leaders"][1] == G and r["replicas"][1] == 0 and r["commits"][1] == 0  # (a zero shadow says vacant: every slot is news)
    for e in (s, one):
        elect((e,), np.arange(G), 10)
        dtick((e,), 3, lambda k, head, slot: head)
        dtick((e,), 1, lambda k, head, slot: np.where(np.arange(G) % 3 == 0, capi.NO_ACK, head).astype(np.uint64))
    peeks = dict(leaders=dict(peek=True), replicas=dict(LAGS, peek=True), commits=dict(peek=True, backlog=True), census=True, repl_census=0)
    both(s, one, "a range across the shard border", how, g0=first - 5, n=11, **peeks)
    both(s, one, "a range inside the last shard", how, g0=s.shard(D - 1).group_lo + 1, n=9, **peeks)
    # the caps run out inside shard 0 for the leaders, inside shard 1 for the commits, not at all for the replicas
    r = both(s, one, "caps that end in different shards", how, leaders=dict(limit=first // 2), replicas=dict(LAGS),
             commits=dict(limit=first + (second - first) // 2, backlog=True), census=True, repl_census=0)
    assert r["leaders"][0]["group"][-1] == first // 2 - 1 and first <= r["commits"][0]["group"][-1] < second - 1 and len(r["replicas"][0]) == G
    r = both(s, one, "the shards behind a cap kept that feed's shadow", how, **peeks)
    assert r["leaders"][1] == G - first // 2 and r["commits"][1] == G - first - (second - first) // 2 and r["replicas"][1] == 0
    for e in (s, one):
        dtick((e,), 2, lambda k, head, slot: np.where((k == 1) & (np.arange(G) % 2 == 0), capi.NO_ACK, head).astype(np.uint64))
        e.close_groups(np.sort(np.random.default_rng(5).choice(G, 100, replace=False)))
    both(s, one, "caps of 1, 0 and commits only", how, leaders=dict(limit=1), replicas=dict(LAGS, limit=0), commits=dict(commits_only=True, limit=second))
    both(s, one, "a cap at the shard border", how, leaders=dict(limit=first - first // 2 - 1), replicas=dict(LAGS, limit=first, peek=True), commits=dict(limit=3))
    r = both(s, one, "the rest", how, **EVERYTHING)
    assert all(r[k][1] > 0 and (np.diff(r[k][0]["group"].astype(np.int64)) > 0).all() for k in FEEDS)
    assert all(v[1] == 0 for k, v in both(one, s, "quiet", how, **EVERYTHING).items() if k in FEEDS)
    compare_snapshots(s, one, "shards")


# ---- 9. a node of a dense cluster, between rounds ----------------------------------------------------------------------------
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
            r = both(libs[0][1][k], libs[1][1][k], f"poll {p} node {k}", (calls, poll) if (p + k) % 2 else (poll, calls), **EVERYTHING)
            rows += r["commits"][1]
            assert r["census"]["leaders"] > 0 and r["census"]["followers"] > 0
    assert rows > G
    for lib, _ in libs:
        lib.close()


# ---- 10. launches ------------------------------------------------------------------------------------------------------------
def test_small_launches():
    G, R = G_SMALL, 3
    a, b = twins(G, R, 8)
    busy((a, b), G, R, wide_lag=False)
    feeds = dict(leaders={}, replicas=dict(LAGS), commits=dict(backlog=True))
    for what in ("everything moved", "quiet"):
        la, lb = a.counters()["launches"], b.counters()["launches"]
        both(a, b, what, **feeds)
        la, lb = a.counters()["launches"] - la, b.counters()["launches"] - lb
        assert lb < la, (what, la, lb)  # one count pass and one scan instead of three of each
        assert (la, lb) == (10, 6), (what, la, lb)


# The six separate calls are served by the poll's host path; what each queues is pinned here, per call, as the numbers the
# calls had when each had a chain of its own.  One device: a count pass, the scan and - with a cap - the write pass; a
# backlog is one launch more; a census is two.  Two shards: every shard is sized (no write pass), then the shards that have
# rows within the cap deliver - a limit that ends inside shard 0 leaves shard 1 uncalled the second time.
SEPARATE_LAUNCHES = {
    1: dict(leaders=(2, 3, 3, 3), replicas=(2, 3, 3, 3), timed=(2, 3, 3, 3), commits=(2, 3, 3, 3), commits_backlog=(3, 4, 4, 4), census=2, repl_census=2),
    2: dict(leaders=(4, 7, 10, 4), replicas=(4, 7, 10, 4), timed=(4, 7, 10, 4), commits=(4, 7, 10, 4), commits_backlog=(6, 9, 12, 6), census=4, repl_census=4),
}


@pytest.mark.parametrize("D", [pytest.param(1, id="small-one-device"), pytest.param(2, id="small-two-shards")])
def test_launches_of_the_separate_calls(D):
    G, R = 200, 3
    inside = 50  # a limit that ends inside shard 0 (100 slots)

    def engine():
        e = BatchedRaft(G, R, seed=9, **(dict(device_ids=[0] * D) if D > 1 else {}))
        busy((e,), G, R, wide_lag=False)
        return e

    def launched(e, call):
        before = e.counters()["launches"]
        r = call()
        return e.counters()["launches"] - before, r

    feeds = dict(
        leaders=lambda e, **kw: e.watch_leaders(**kw),
        replicas=lambda e, **kw: e.watch_replicas(2, 0, **kw),
        timed=lambda e, **kw: e.watch_replicas_timed(5000, 100, **kw),
        commits=lambda e, **kw: e.watch_commits(**kw),
        commits_backlog=lambda e, **kw: e.watch_commits(backlog=True, **kw),
    )
    got = {}
    for name, call in feeds.items():
        e = engine()  # (a feed of its own engine: every slot is news to it)
        assert D == 1 or e.shard(0).G > inside
        ls = []
        for what, kw, total in (("limit=0", dict(limit=0), G), ("a limit inside shard 0", dict(limit=inside), G), ("moved", {}, G - inside),
                                ("quiet", {}, 0)):
            k, r = launched(e, lambda: call(e, **kw))
            assert r[1] == total and len(r[0]) == min(kw.get("limit", G), total), (name, what, r[1], len(r[0]))
            ls.append(k)
        got[name] = tuple(ls)
    e = engine()
    got["census"] = launched(e, e.census)[0]
    got["repl_census"] = launched(e, lambda: e.replication_census(1))[0]
    print("launches of the separate calls:", D, got)
    assert got == SEPARATE_LAUNCHES[D], (D, got)


# ---- 11. the stride (the device only) ----------------------------------------------------------------------------------------
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
    r = both(a, b, "everything moved", **EVERYTHING)
    assert r["leaders"][1] == G and r["commits"][1] == G
    moved = rng.random(G) < 0.01
    silent = lambda k, head, slot: np.where(k == 1, capi.NO_ACK, head).astype(np.uint64)  # noqa: E731
    dtick((a, b), np.where(moved, 2, 0), silent)
    dtick((a, b), 0, silent)
    r = both(a, b, "one percent", leaders={}, replicas=dict(leave_lag=1, join_lag=0), commits=dict(limit=5000, backlog=True), census=True, repl_census=1)
    assert r["commits"][1] == int(moved.sum()) and len(r["commits"][0]) == 5000 and r["commits"][2]["appended"] == int(moved.sum())
    assert r["replicas"][1] > 0 and r["leaders"][1] == 0
    r = both(a, b, "the rest of it", (poll, calls), **EVERYTHING)
    assert r["commits"][1] == int(moved.sum()) - 5000
