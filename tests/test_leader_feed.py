"""The leadership feed and the census (ABI v14): jg_engine_watch_leaders / jg_engine_census.  The leadership view of a
slot - role, term, known leader, fault, vacancy - is a function of columns jg_read_state exposes, so the expected rows
are stated twice: in numpy over the engine's own read(...) columns, and over tests/ref_py fed the same batches.  A watch
returns exactly the slots whose view differs from what it last delivered; a census equals the numpy counts; neither
changes anything a step, a drain or a read can observe.  Cases whose id contains "small" are small enough for the
emulated device (tests/test_leader_feed_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, capi, move_groups
from josefine_amd.engine import EngineError
from fuzz import random_batch
from parity import compare_drains, compare_snapshots
from ref_py.engine import RefEngine
from test_move_groups import drain_all
from test_vacant_groups import DRAINS, drains_without, fresh, records

pytestmark = pytest.mark.gpu

VAC = capi.FAULT_VACANT
KNOWN, SELF, VACANT, FAULTED = capi.LEAD_KNOWN, capi.LEAD_SELF, capi.LEAD_VACANT, capi.LEAD_FAULTED
WATCH_TILE = 256 * 4    # slots per workgroup of the watch passes (jg_watch.h JG_WATCH_TILE)
CENSUS_TILE = 256 * 16  # ... of the census pass (JG_CENSUS_TILE)
COMPARED = ("leader_id", "term", "role", "state", "fault")  # a slot differs in any field but group / self_slot
KINDS = ("became leader", "learned a leader", "lost the leader to candidacy", "term changed with the leader unchanged",
         "faulted", "closed", "opened")


def view_of(e, g0=0, n=None, vacant=None):
    """the leadership view of slots g0 .. g0 + n - 1 from e.read(...) (a BatchedRaft or a RefEngine; `vacant`: the slots
    that are closed on the engine the RefEngine shadows, which itself knows no vacancy)"""
    n = e.G - g0 if n is None else n
    col = {k: e.read(k, 0, g0, n) for k in ("role", "term", "leader_id", "has_leader", "fault", "self_slot")}
    ids = np.array(e.node_ids, np.uint32)
    v = np.zeros(n, capi.LEADER_ROW_DTYPE)
    v["group"] = g0 + np.arange(n)
    v["self_slot"] = col["self_slot"]
    lead = col["role"] == capi.ROLE_LEADER
    known = col["has_leader"] == 1  # (read as 1 only for a follower)
    v["role"], v["term"], v["fault"] = col["role"], col["term"], col["fault"]
    v["leader_id"] = np.where(lead, ids[col["self_slot"]], np.where(known, col["leader_id"], 0))
    v["state"] = np.where(lead, KNOWN | SELF, np.where(known, KNOWN, 0)) | np.where(col["fault"] != 0, FAULTED, 0)
    vac = col["fault"] == VAC
    if vacant is not None:
        vac = vac | np.isin(v["group"], vacant)
    for k, x in (("role", 0), ("term", 0), ("leader_id", 0), ("state", VACANT), ("fault", VAC)):
        v[k][vac] = x
    return v


def never_reported(e, g0=0, n=None):
    """what a watch starts from: every slot last reported vacant"""
    n = e.G - g0 if n is None else n
    v = np.zeros(n, capi.LEADER_ROW_DTYPE)
    v["group"], v["state"], v["fault"] = g0 + np.arange(n), VACANT, VAC
    return v


def differs(a, b):
    m = np.zeros(len(a), bool)
    for k in COMPARED:
        m |= a[k] != b[k]
    return m


def classify(prev, cur, kinds):
    """the kinds of transition in the expected stream prev -> cur (the slots that differ)"""
    pk, ck = (prev["state"] & KNOWN) != 0, (cur["state"] & KNOWN) != 0
    tests = {
        "became leader": ((cur["state"] & SELF) != 0) & ((prev["state"] & SELF) == 0),
        "learned a leader": ck & ((cur["state"] & SELF) == 0) & (~pk | (prev["leader_id"] != cur["leader_id"])),
        "lost the leader to candidacy": pk & (cur["role"] == capi.ROLE_CANDIDATE) & ((cur["state"] & VACANT) == 0),
        "term changed with the leader unchanged": pk & ck & (prev["leader_id"] == cur["leader_id"]) & (prev["term"] != cur["term"]),
        "faulted": ((cur["state"] & FAULTED) != 0) & ((prev["state"] & FAULTED) == 0),
        "closed": ((cur["state"] & VACANT) != 0) & ((prev["state"] & VACANT) == 0),
        "opened": ((prev["state"] & VACANT) != 0) & ((cur["state"] & VACANT) == 0),
    }
    for k, m in tests.items():
        if m.any():
            kinds.add(k)


def census_np(e, g0=0, n=None):
    """jg_census over slots g0 .. g0 + n - 1 from e.read(...)"""
    n = e.G - g0 if n is None else n
    v = view_of(e, g0, n)
    hosted = v["fault"] != VAC
    ok = hosted & (v["fault"] == 0)
    known = ok & ((v["state"] & KNOWN) != 0)
    ids = np.array(e.node_ids[:e.R], np.uint32)
    lead = ok & (v["role"] == capi.ROLE_LEADER)
    head, commit = e.read("head", 0, g0, n), e.read("commit", 0, g0, n)
    return dict(hosted=int(hosted.sum()), vacant=int((~hosted).sum()),
                faulted_reference=int((hosted & (v["fault"] >= 1) & (v["fault"] < 128)).sum()),
                faulted_engine=int((hosted & (v["fault"] >= 128)).sum()),
                followers=int((ok & (v["role"] == capi.ROLE_FOLLOWER)).sum()),
                candidates=int((ok & (v["role"] == capi.ROLE_CANDIDATE)).sum()), leaders=int(lead.sum()),
                leaderless=int((ok & ~known).sum()), led_by=[int((known & (v["leader_id"] == i)).sum()) for i in ids],
                led_by_other=int((known & ~np.isin(v["leader_id"], ids)).sum()),
                max_term=int(v["term"][hosted].max()) if hosted.any() else 0,
                uncommitted=int((head[lead] - commit[lead]).sum(dtype=np.uint64)))


class Feed:
    """the test's statement of one engine's feed: `seen` is the view the watch last delivered per slot"""

    def __init__(self, e):
        self.e, self.seen, self.kinds = e, never_reported(e), set()

    def expect(self):
        cur = view_of(self.e)
        return cur, differs(self.seen, cur)

    def check(self, what="", ref=None, vacant=None):
        """a watch of the whole engine returns exactly the pending slots, ascending, as their current view - which is
        ref's; a second watch returns nothing; the census is numpy's"""
        cur, m = self.expect()
        if ref is not None:
            want = view_of(ref, vacant=vacant)
            assert cur.tobytes() == want.tobytes(), (what, np.nonzero(differs(cur, want))[0][:8])
        rows, total = self.e.watch_leaders()
        assert total == int(m.sum()) and rows.tobytes() == cur[m].tobytes(), (what, total, int(m.sum()))
        classify(self.seen[m], cur[m], self.kinds)
        self.seen = cur
        rows, total = self.e.watch_leaders()
        assert total == 0 and len(rows) == 0, what
        assert self.e.census() == census_np(self.e), what
        return int(m.sum())


def history(G, R, seed, steps, close_at=None, open_at=None, recreate=0.01):
    """a fuzzed history on an engine and ref_py, the feed checked after every step; at close_at a quarter of the slots is
    closed on the engine (ref_py's copies go on), at open_at they are reopened (ref_py: re-created with the carried draws)"""
    rng = np.random.default_rng(seed)
    slots = rng.integers(0, R, G).astype(np.uint8)
    a, kw = fresh(G, R, R + seed, slots)
    ref = RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    feed = Feed(a)
    assert feed.check("fresh", ref) == G  # a fresh hosted engine: every slot once, followers at term 0
    closed, hosted, draws, now = np.zeros(0, np.int64), np.arange(G), None, 0
    for s in range(steps):
        if s == close_at:
            closed = np.sort(rng.choice(G, G // 4, replace=False))
            a.close_groups(closed)
            draws = records(a)[closed, 10] >> 32
            assert feed.check(f"close {s}", ref, closed) == (feed.seen["state"][closed] & VACANT != 0).sum() == len(closed)
        if s == open_at:
            now += 1000
            a.open_groups(closed, now)
            for g, d in zip(closed, draws):
                ref.draws[int(g)] = int(d)
                ref.submit(int(g), Command.Recreate())
            ref.step(now)
            drain_all(ref)
            budget[closed] = capi.CHAIN_WINDOW - 2
            n = feed.check(f"open {s}", ref)
            assert n == len(closed) and (feed.seen["term"][closed] == 0).all() and (feed.seen["state"][closed] == 0).all()
            closed = np.zeros(0, np.int64)
        batch = random_batch(rng, ref, 3 * G, foreign_voters=True, budget=budget)
        now += int(rng.integers(0, 300))
        rec = np.nonzero(rng.random(G) < recreate)[0]
        for e in (a, ref):
            e.submit_columns(**batch)
            for g in rec:
                e.submit(int(g), Command.Recreate())
            e.step(now)
        drains_without(a, {fn: getattr(ref, fn)() for fn in DRAINS}, closed, f"step {s}")
        feed.check(f"step {s}", ref, closed)
    return feed, a, ref


# ---- 1. exactness, 2. every kind of transition occurs ---------------------------------------------------------------
@pytest.mark.parametrize("G,R,seed", [pytest.param(192, 3, 1, id="small-3"), pytest.param(160, 5, 2, id="small-5")])
def test_exact_feed(G, R, seed):
    feed, a, ref = history(G, R, seed, 40, close_at=14, open_at=26)
    compare_snapshots(a, ref, "after the history")
    # every kind of transition of the issue's list is in the expected stream of each case (all can occur under the
    # fuzzers: none is excused)
    assert feed.kinds == set(KINDS), sorted(set(KINDS) - feed.kinds)


# ---- 3. cap -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", [pytest.param(1, id="small-1"), pytest.param(7, id="small-7"), pytest.param(None, id="small-half")])
def test_cap(limit):
    from josefine_amd.traces import elect_all
    G, R = 150, 3
    e = BatchedRaft(G, R, seed=3, self_slots=(np.arange(G) % R).astype(np.uint8))
    feed = Feed(e)
    elect_all(e, 10)
    drain_all(e)
    limit = G // 2 if limit is None else limit
    cur, m = feed.expect()
    pending = int(m.sum())
    assert pending == G
    # a peek delivers the same rows and advances nothing
    for _ in range(2):
        rows, total = e.watch_leaders(limit=limit, peek=True)
        assert total == pending and rows.tobytes() == cur[m][:limit].tobytes()
    got, touched = [], False
    while True:
        rows, total = e.watch_leaders(limit=limit)
        assert total == pending and len(rows) == min(limit, pending)
        cur, m = feed.expect()
        assert rows.tobytes() == cur[m][:limit].tobytes()
        feed.seen[rows["group"]] = rows
        got.append(rows)
        pending -= len(rows)
        if not pending:
            break
        if not touched and len(np.concatenate(got)) >= 8:
            # between two chunks a delivered slot and a pending one change (re-created: followers at term 0 again)
            touched = True
            for g in (0, G - 1):
                e.submit(g, Command.Recreate())
            e.step(2000)
            drain_all(e)
            pending += 1  # slot 0 is pending again; slot G - 1 still is, and is reported with its newest view
    for r in got:
        assert (np.diff(r["group"].astype(np.int64)) > 0).all()
    allrows = np.concatenate(got)
    seq = allrows["group"].astype(np.int64)
    back = np.nonzero(np.diff(seq) <= 0)[0]
    assert len(back) == 1 and seq[back[0] + 1] == 0  # ascending chunks; slot 0 alone came a second time
    assert np.bincount(allrows["group"], minlength=G).tolist() == [2] + [1] * (G - 1)  # every pending slot exactly once
    for g in (0, G - 1):
        last = allrows[allrows["group"] == g][-1]
        assert last["role"] == capi.ROLE_FOLLOWER and last["term"] == 0 and last["state"] == 0, g
    assert allrows[allrows["group"] == 0][0]["state"] == KNOWN | SELF
    assert e.watch_leaders()[1] == 0
    assert differs(feed.seen, view_of(e)).sum() == 0


# ---- 4. watching changes nothing --------------------------------------------------------------------------------------
def same_drains(a, b, ref, what):
    for fn in DRAINS:
        want = getattr(ref, fn)()
        for e in (a, b):
            got = getattr(e, fn)()
            assert got.tobytes() == want.tobytes(), (what, fn, len(got), len(want))


def test_small_watching_changes_nothing():
    G, R = 128, 3
    rng = np.random.default_rng(11)
    slots = rng.integers(0, R, G).astype(np.uint8)
    a, kw = fresh(G, R, 5, slots)
    b, _ = fresh(G, R, 5, slots)
    ref = RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    feed = Feed(a)

    def look(what):
        feed.check(what)
        a.watch_leaders(10, 50, limit=3, peek=True)
        a.census(7, 99)

    look("fresh")
    now = 0
    for s in range(16):  # the general state machine, against the twin and ref_py
        batch = random_batch(rng, ref, 3 * G, foreign_voters=True, budget=budget)
        now += int(rng.integers(0, 300))
        for e in (a, b, ref):
            e.submit_columns(**batch)
            e.step(now)
        look(f"step {s}")
        same_drains(a, b, ref, f"step {s}")
        compare_snapshots(a, ref, f"step {s}")
    for t in range(4):  # dense ticks: the leaders append, the others take an engine-domain fault
        acks = np.full((R, G), capi.NO_ACK, np.uint64)
        some = rng.random(G) < 0.3
        acks[slots[some].astype(np.int64), np.nonzero(some)[0]] = 3
        for e in (a, b, ref):
            e.step_dense_acks(acks)
        look(f"dense {t}")
        same_drains(a, b, ref, f"dense {t}")
        compare_snapshots(a, ref, f"dense {t}")
    compare_snapshots(a, b, "twin")
    # node steps (ref_py has no node step: the unwatched twin alone), JG_NODE_ASYNC: the watch settles the step
    for t in range(8):
        now += int(rng.integers(100, 400))
        batch = random_batch(rng, b, G, foreign_voters=True, budget=budget)
        outs = []
        for e in (a, b):
            e.submit_columns(**batch)
            e.step_node_begin(now, async_=True)
            if e is a:
                look(f"node {t}")
            outs.append(e.node_outbox())
        for name, x in outs[0].items():
            assert np.array_equal(np.asarray(x), np.asarray(outs[1][name])), (t, name)
        look(f"node {t} after")
        compare_drains(a, b, f"node {t}")
        compare_snapshots(a, b, f"node {t}")
    assert a.read_chains()["off"].tobytes() == b.read_chains()["off"].tobytes()


# ---- 5. the control plane, seen through the diff alone ---------------------------------------------------------------
def test_small_control_plane():
    from node_step import elect_some
    G, R = 192, 3
    src = BatchedRaft(G, R, seed=2)
    fs = Feed(src)
    assert fs.check("fresh") == G  # a fresh hosted engine: G rows once
    assert (fs.seen["role"] == capi.ROLE_FOLLOWER).all() and (fs.seen["term"] == 0).all() and (fs.seen["state"] == 0).all()
    elect_some(src, np.arange(G) < 96, now_ms=10)  # slots 0 .. 95 lead
    drain_all(src)
    assert fs.check("elected") == 96
    assert (fs.seen["state"][:96] == (KNOWN | SELF)).all() and (fs.seen["leader_id"][:96] == src.node_ids[0]).all()
    # start_vacant: nothing until slots are opened; open: follower rows at term 0
    dst = BatchedRaft(G, R, seed=2, start_vacant=True)
    fd = Feed(dst)
    assert dst.watch_leaders() [1] == 0 and fd.check("start vacant") == 0
    dst.open_groups(range(150, 160), 500)
    rows, total = dst.watch_leaders(peek=True)
    assert total == 10 and rows["group"].tolist() == list(range(150, 160))
    assert (rows["role"] == capi.ROLE_FOLLOWER).all() and (rows["term"] == 0).all() and (rows["state"] == 0).all() and (rows["fault"] == 0).all()
    assert fd.check("opened") == 10
    # a move of leaders and followers: KNOWN | SELF rows on the destination, VACANT rows on the source
    move_groups(src, dst, 80, 30, close_source=True)
    rows, total = dst.watch_leaders(peek=True)
    assert total == 30 and rows["group"].tolist() == list(range(80, 110))
    assert (rows["state"][:16] == (KNOWN | SELF)).all() and (rows["term"][:16] == 1).all() and (rows["state"][16:] == 0).all()
    assert fd.check("imported") == 30
    rows, total = src.watch_leaders(peek=True)
    assert total == 30 and (rows["state"] == VACANT).all() and (rows["fault"] == VAC).all() and (rows["term"] == 0).all()
    assert fs.check("moved away") == 30
    # close: VACANT rows; load_chains: follower rows at term 0 (slots 0 .. 9 led at term 1 before)
    src.close_groups(range(120, 130))
    rows, total = src.watch_leaders(peek=True)
    assert total == 10 and (rows["state"] == VACANT).all()
    assert fs.check("closed") == 10
    trees = [([(0, 0)] + [(i, i - 1) for i in range(1, k + 2)], k) for k in range(10)]
    src.load_chains(trees, now_ms=100)
    rows, total = src.watch_leaders(peek=True)
    assert total == 10 and rows["group"].tolist() == list(range(10))
    assert (rows["role"] == capi.ROLE_FOLLOWER).all() and (rows["term"] == 0).all() and (rows["state"] == 0).all()
    assert fs.check("loaded") == 10
    src.load_chains(trees, now_ms=100, g0=120)  # ... and a load opens a vacant range
    assert fs.check("loaded over vacant slots") == 10


# ---- 6. census --------------------------------------------------------------------------------------------------------
def check_census(e, what=""):
    G = e.G
    cuts = [(0, G), (1, G - 1), (3, 0), (G - 5, 5), (G // 3, G // 2), (0, CENSUS_TILE), (7, CENSUS_TILE - 1), (5, CENSUS_TILE + 1),
            (CENSUS_TILE - 3, 7), (WATCH_TILE - 1, WATCH_TILE + 1)]
    for g0, n in cuts:
        if g0 + n <= G:
            assert e.census(g0, n) == census_np(e, g0, n), (what, g0, n)


def test_small_census():
    from node_step import elect_some
    G, R = CENSUS_TILE + 300, 5
    rng = np.random.default_rng(9)
    slots = rng.integers(0, R, G).astype(np.uint8)
    e = BatchedRaft(G, R, seed=4, self_slots=slots)
    check_census(e, "fresh")
    lead = rng.random(G) < 0.5
    elect_some(e, lead, now_ms=10)
    # followers that know a leader: a Heartbeat from a member, and from a node outside the membership
    fol = np.nonzero(~lead)[0].astype(np.uint32)
    hb = fol[: len(fol) // 2]
    frm = np.where(np.arange(len(hb)) % 7 == 0, 77, np.array(e.node_ids, np.uint32)[(slots[hb].astype(np.int64) + 1) % R]).astype(np.uint32)
    e.submit_columns(np.full(len(hb), capi.CMD_HEARTBEAT, np.uint8), hb, from_=frm, term=np.full(len(hb), 3, np.uint64))
    e.submit_columns(np.full(20, capi.CMD_TIMEOUT, np.uint8), fol[-20:])  # candidates
    e.step(20)
    drain_all(e)
    check_census(e, "elected")
    c = e.census()
    assert c["candidates"] == 20 and c["led_by_other"] > 0 and c["leaderless"] > 0 and min(c["led_by"]) > 0 and c["max_term"] == 3
    # a dense tick: the leaders append 1100 blocks nobody acknowledges - at R = 5 the commit's lag leaves its 10-bit field
    # (the escape storage); a few non-leaders take an engine-domain fault
    acks = np.full((R, G), capi.NO_ACK, np.uint64)
    some = lead | (rng.random(G) < 0.02)
    acks[slots[some].astype(np.int64), np.nonzero(some)[0]] = np.where(lead[some], 1100, 0).astype(np.uint64)
    e.step_dense_acks(acks)
    drain_all(e)
    role = e.read("role")
    gap = (e.read("head") - e.read("commit"))[role == capi.ROLE_LEADER]
    assert (gap >= (1 << (64 // (R + 1))) - 2).all() and len(gap) > 100  # every leader's commit sits in the escape storage
    c = e.census()
    assert c["uncommitted"] == int(gap.sum()) and c["faulted_engine"] > 0
    check_census(e, "escaped")
    # reference-domain faults (an AppendResponse from a node the leader's progress does not know, progress.rs:43), and
    # vacant slots
    g = np.nonzero(lead)[0][:9].astype(np.uint32)
    e.submit_columns(np.full(9, capi.CMD_APPEND_RESPONSE, np.uint8), g, from_=np.full(9, 77, np.uint32), term=np.ones(9, np.uint64),
                     id=np.ones(9, np.uint64), flag=np.ones(9, np.uint8))
    e.step(10_000)
    assert e.census()["faulted_reference"] == 9
    e.close_groups(np.sort(rng.choice(G, G // 5, replace=False)))
    drain_all(e)
    check_census(e, "vacant and faulted")
    c = e.census()
    assert c["vacant"] == G // 5 and c["hosted"] == G - G // 5
    v = BatchedRaft(300, 3, seed=1, start_vacant=True)
    assert v.census() == census_np(v) and v.census()["max_term"] == 0 and v.census()["vacant"] == 300


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_small_refusals():
    G, R = 200, 3
    e, twin = BatchedRaft(G, R, seed=4), BatchedRaft(G, R, seed=4)
    api, h = e.api, e._h
    rows = np.zeros(G, capi.LEADER_ROW_DTYPE)
    total, c = C.c_size_t(0), capi.Census()
    watch = lambda flags, g0, n, out, cap, tot: api.engine_watch_leaders(h, flags, g0, n, out, cap, tot)  # noqa: E731
    assert watch(0, 0, G, rows.ctypes.data, G, None) == capi.EINVAL            # a null total
    assert watch(0, 0, G, None, 5, C.byref(total)) == capi.EINVAL              # a null out with cap > 0
    assert watch(2, 0, G, rows.ctypes.data, G, C.byref(total)) == capi.EINVAL  # an unknown flag
    assert watch(0, G - 1, 2, rows.ctypes.data, G, C.byref(total)) == capi.EINVAL
    assert watch(0, 1, 0xFFFFFFFF, rows.ctypes.data, G, C.byref(total)) == capi.EINVAL
    assert api.engine_census(h, 0, G, None) == capi.EINVAL
    assert api.engine_census(h, G, 1, C.byref(c)) == capi.EINVAL
    assert watch(capi.WATCH_PEEK, 0, G, None, 0, C.byref(total)) == capi.OK and total.value == G  # nothing was advanced
    # kept node steps outstanding: refused with read_chains's code, and the kept steps are still viewable afterwards
    for x in (e, twin):
        x.step_node_begin(1000, async_=True, keep=True)
        x.step_node_begin(1100, async_=True, keep=True)
    r = capi.ChainRead()
    r.n, off = G, np.zeros(G + 1, np.uint64)
    r.off = off.ctypes.data
    code = api.engine_read_chains(h, C.byref(r), C.byref(C.c_uint64(0)))
    assert code == capi.EINVAL
    assert watch(0, 0, G, rows.ctypes.data, G, C.byref(total)) == code and api.engine_census(h, 0, G, C.byref(c)) == code
    with pytest.raises(EngineError):
        e.watch_leaders()
    outs = [[x.node_outbox(), x.node_outbox()] for x in (e, twin)]
    for k in range(2):
        for name, v in outs[0][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][k][name])), (k, name)
    compare_drains(e, twin, "kept")
    compare_snapshots(e, twin, "kept")
    assert e.watch_leaders()[1] == G and e.census() == census_np(e)


# ---- 8. shards --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [pytest.param(2, id="small-2-shards"), pytest.param(3, id="small-3-shards")])
def test_shards(D):
    from node_step import elect_some
    G, R = 1000, 3
    rng = np.random.default_rng(D)
    s = BatchedRaft(G, R, seed=4, device_ids=[0] * D)
    one = BatchedRaft(G, R, seed=4)
    last = s.shard(D - 1).group_lo

    def same(what, **kw):
        a, b = s.watch_leaders(**kw), one.watch_leaders(**kw)
        assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes(), (what, kw, a[1], b[1])
        return a

    same("fresh, count", limit=0)
    same("fresh, range", g0=300, n=500, peek=True)
    first = s.shard(0).G
    rows, total = same("a limit that ends inside the first shard", limit=first // 2)
    assert total == G and rows["group"].tolist() == list(range(first // 2))
    rows, total = same("the rest")
    assert total == G - first // 2 and rows["group"][0] == first // 2 and rows["group"][-1] == G - 1
    assert same("quiet")[1] == 0
    gs = np.sort(rng.choice(G, 400, replace=False))
    for e in (s, one):
        elect_some(e, np.isin(np.arange(G), gs[::2]), now_ms=10)
        e.close_groups(gs[1::2])
        drain_all(e)
    for g0, n in ((0, G), (1, last + 3), (last - 2, 7), (G - 1, 1), (0, 0)):
        assert s.census(g0, n) == one.census(g0, n) == census_np(one, g0, n), (g0, n)
    same("peek", peek=True, limit=7)
    rows, total = same("a limit of 1", limit=1)
    same("the last shard alone", g0=last, n=G - last, limit=3)
    rows, total = same("the rest")
    assert total == 400 - 1 - 3
    assert same("quiet")[1] == 0
    compare_snapshots(s, one, "shards")


# ---- 9. full size (the device only) ----------------------------------------------------------------------------------
def test_any_leader_cluster_1m():
    from josefine_amd import DenseCluster
    from test_any_leader import spread_leaders
    G, R = 1 << 20, 3
    nodes = [BatchedRaft(G, R, seed=5 + r, self_slots=np.full(G, r, np.uint8), flags=capi.CFG_SEPARATE_COMMIT_KEY) for r in range(R)]
    spread_leaders(nodes, G, R)
    lib = DenseCluster(nodes, lead=None)
    lib.set_appends(1)
    lib.rounds(100, 100, 6)  # the followers learn their leaders from the first Heartbeat
    cs = [e.census() for e in nodes]
    for k, c in enumerate(cs):
        print(f"node {k}: {c}")
    assert sum(c["leaders"] for c in cs) == G
    assert all(c["led_by"] == cs[0]["led_by"] for c in cs) and sum(cs[0]["led_by"]) == G
    assert all(c["leaderless"] == 0 and c["hosted"] == G and c["led_by_other"] == 0 for c in cs)
    assert all(c == census_np(e) for c, e in zip(cs, nodes))
    for k, e in enumerate(nodes):
        rows, total = e.watch_leaders()
        want = view_of(e)
        assert total == G and rows.tobytes() == want.tobytes(), k
        mine = rows["group"][(rows["state"] & SELF) != 0]
        assert np.array_equal(mine, np.nonzero(e.read("role") == capi.ROLE_LEADER)[0]), k
        assert (rows["leader_id"] == np.array(e.node_ids, np.uint32)[np.arange(G) % R]).all(), k
    # the quiet feed: one more round of steady appends changes no slot's view
    lib.rounds(700, 100, 1)
    for k, e in enumerate(nodes):
        assert e.watch_leaders() [1] == 0, k
        assert e.census()["uncommitted"] == census_np(e)["uncommitted"], k
    lib.close()


def test_watch_16m():
    G = 1 << 24
    rng = np.random.default_rng(6)
    e = BatchedRaft(G, 1, seed=1, start_vacant=True)
    assert e.watch_leaders(limit=0)[1] == 0
    gs = np.nonzero(rng.random(G) < 1 / 4.5)[0].astype(np.uint32)  # a random ascending 1 / 4.5 of the slots
    e.open_groups(gs)
    want = np.zeros(gs.size, capi.LEADER_ROW_DTYPE)
    want["group"] = gs
    rows, total = e.watch_leaders(limit=1000, peek=True)
    assert total == gs.size and rows.tobytes() == want[:1000].tobytes()
    rows, total = e.watch_leaders(G // 2, G // 4, limit=G // 8)
    part = want[(gs >= G // 2) & (gs < G // 2 + G // 4)]
    assert total == len(part) and rows.tobytes() == part.tobytes()
    rows, total = e.watch_leaders(limit=gs.size)
    rest = want[~np.isin(gs, part["group"])]
    assert total == len(rest) and rows.tobytes() == rest.tobytes()
    assert e.watch_leaders(limit=0)[1] == 0
    c = e.census()
    assert c["hosted"] == gs.size and c["vacant"] == G - gs.size and c["followers"] == gs.size and c["leaderless"] == gs.size
