"""The replication feed and its census (ABI v15): jg_engine_watch_replicas / jg_engine_replication_census.  The replication
view of a slot - which members of a partition this engine leads are in sync - is a function of columns jg_read_state
exposes (role, fault, self slot, head, commit, match of every member, the Replicate mask) and of what the feed last
delivered (the hysteresis), so the expected rows are stated in numpy over the engine's own read(...) columns and a `seen`
array, and again over tests/ref_py fed the same batches where ref_py can run the scenario.  A watch returns exactly the
slots whose (isr, LEADS) differs from what it last delivered, ascending, every field equal; a census equals the numpy
counts; neither changes anything a step, a drain or a read can observe.  Cases whose id contains "small" are small enough
for the emulated device (tests/test_replica_feed_emulated.py).

"Lost leadership to a higher term" is NOT a conversion to follower here: the reference's Leader::term is unimplemented!()
(leader.rs:33-35), so a leader that meets a higher term stops at that term with JG_FAULT_LEADER_TERM_UNIMPLEMENTED and its
role column stays leader.  The feed reports LEADS gone; the test records that row under this name when the slot's term
rose, and under "faulted" when it did not."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, capi, move_groups
from josefine_amd.engine import EngineError
from fuzz import random_batch
from parity import compare_drains, compare_snapshots
from ref_py.engine import RefEngine
from test_move_groups import drain_all
from test_vacant_groups import DRAINS, fresh

pytestmark = pytest.mark.gpu

VAC = capi.FAULT_VACANT
LEADS, UNDER, BELOW = capi.ISR_LEADS, capi.ISR_UNDER, capi.ISR_BELOW_QUORUM
ISR_TILE = 256 * 4     # slots per workgroup of the watch passes (jg_isr.h JG_ISR_TILE)
SEEN_LEADS = 0x100     # `seen`: isr | SEEN_LEADS where the slot was last reported leading
U64_MAX = (1 << 64) - 1
KINDS = ("became leader", "follower joined", "follower left", "follower rejoined", "went below quorum",
         "lost leadership to a higher term", "closed", "opened", "faulted")


def popcount8(x):
    return np.unpackbits(np.asarray(x, np.uint8)[:, None], axis=1).sum(axis=1)


def lags_of(e, g0, n):
    """(leads, head, [R][n] saturating lags with the own slot's 0, own-slot masks) of slots g0 .. g0 + n - 1"""
    role, fault, slot = e.read("role", 0, g0, n), e.read("fault", 0, g0, n), e.read("self_slot", 0, g0, n)
    head = e.read("head", 0, g0, n).astype(np.uint64)
    leads = (role == capi.ROLE_LEADER) & (fault == 0)
    lag = np.zeros((e.R, n), np.uint64)
    for r in range(e.R):
        match = e.read("match", r, g0, n).astype(np.uint64)
        lag[r] = np.where((head > match) & (slot != r), head - np.minimum(match, head), 0)
    return leads, head, lag, slot


def view_of(e, seen, leave, join, g0=0, n=None, vacant=None):
    """the replication view of slots g0 .. g0 + n - 1 from e.read(...) (a BatchedRaft or a RefEngine; `vacant`: the slots
    that are closed on the engine the RefEngine shadows) against `seen` (indexed by slot), as rows"""
    n = e.G - g0 if n is None else n
    leads, head, lag, slot = lags_of(e, g0, n)
    if vacant is not None:
        leads = leads & ~np.isin(g0 + np.arange(n), vacant)
    sn = seen[g0:g0 + n]
    was = np.where(sn & SEEN_LEADS, sn & 0xff, 0)
    isr = np.zeros(n, np.uint8)
    for r in range(e.R):
        thr = np.where((was >> r) & 1, np.uint64(leave), np.uint64(join))
        isr |= ((leads & ((slot == r) | (lag[r] <= thr))).astype(np.uint8) << r).astype(np.uint8)
    cnt = popcount8(isr)
    v = np.zeros(n, capi.ISR_ROW_DTYPE)
    v["group"], v["self_slot"], v["isr"] = g0 + np.arange(n), slot, isr
    v["replicate"] = np.where(leads, e.read("repl_state", 0, g0, n), 0)
    v["state"] = np.where(leads, LEADS | np.where(cnt < e.R, UNDER, 0) | np.where(cnt < e.R // 2 + 1, BELOW, 0), 0)
    v["head"] = np.where(leads, head, 0)
    v["worst_lag"] = np.where(leads, lag.max(axis=0), 0)
    return v


def key_of(v):
    """what a watch compares: (isr, LEADS)"""
    return v["isr"].astype(np.uint16) | np.where(v["state"] & LEADS, SEEN_LEADS, 0).astype(np.uint16)


def census_np(e, limit, g0=0, n=None):
    n = e.G - g0 if n is None else n
    leads, head, lag, slot = lags_of(e, g0, n)
    commit = e.read("commit", 0, g0, n).astype(np.uint64)
    lag = np.where(leads, lag, 0).astype(np.uint64)
    out = [(leads & (slot != r) & (lag[r] > np.uint64(limit))) for r in range(e.R)]
    cnt = e.R - np.sum(out, axis=0)
    return dict(leaders=int(leads.sum()), fully_replicated=int((leads & (cnt == e.R)).sum()),
                under_replicated=int((leads & (cnt < e.R)).sum()), below_quorum=int((leads & (cnt < e.R // 2 + 1)).sum()),
                out_of_sync=[int(o.sum()) for o in out], max_lag=[int(lag[r].max()) if n else 0 for r in range(e.R)],
                sum_lag=[int(lag[r].sum(dtype=np.uint64)) for r in range(e.R)],
                max_uncommitted=int((head - commit)[leads].max()) if leads.any() else 0)


def check_census(e, what="", limits=(0, 3, U64_MAX), cuts=None):
    G = e.G
    cuts = cuts or [(0, G), (1, G - 1), (3, 0), (G - 5, 5), (G // 3, G // 2)]
    for g0, n in cuts:
        for limit in limits:
            assert e.replication_census(limit, g0, n) == census_np(e, limit, g0, n), (what, limit, g0, n)


class Feed:
    """the test's statement of one engine's feed: `seen` is the (isr, LEADS) the watch last delivered per slot"""

    def __init__(self, e, leave, join=None):
        self.e, self.leave, self.join = e, leave, leave if join is None else join
        self.seen, self.kinds = np.zeros(e.G, np.uint16), set()
        self.left = np.zeros(e.G, np.uint8)     # the members that have left a slot's set at some time
        self.term = np.zeros(e.G, np.uint64)    # the term a slot was last seen at
        self.closed = np.zeros(e.G, bool)       # the slots that have been reported closed
        self.self_only = 0                      # new leaders reported as {self}

    def expect(self):
        cur = view_of(self.e, self.seen, self.leave, self.join)
        return cur, key_of(cur) != self.seen

    def watch(self, **kw):
        return self.e.watch_replicas(self.leave, self.join, **kw)

    def classify(self, cur, m):
        e = self.e
        prev, key = self.seen, key_of(cur)
        pl, cl = (prev & SEEN_LEADS) != 0, (key & SEEN_LEADS) != 0
        pb, cb = (prev & 0xff).astype(np.uint8), cur["isr"]
        fault, term = e.read("fault"), e.read("term")
        joined, left = cb & ~pb, pb & ~cb
        quorum = e.R // 2 + 1
        tests = {
            "became leader": m & cl & ~pl,
            "follower joined": m & cl & pl & (joined != 0),
            "follower left": m & cl & pl & (left != 0),
            "follower rejoined": m & cl & pl & ((joined & self.left) != 0),
            "went below quorum": m & cl & (popcount8(cb) < quorum) & ~(pl & (popcount8(pb) < quorum)),
            # (a leader that meets a higher term does not become a follower here: the reference's Leader::term is
            # unimplemented!() (leader.rs:33-35), so the replica stops at the new term with JG_FAULT_LEADER_TERM_UNIMPLEMENTED)
            "lost leadership to a higher term": m & pl & ~cl & (fault != VAC) & (term > self.term),
            "closed": m & pl & (fault == VAC),
            "opened": m & cl & self.closed,
            "faulted": m & pl & (fault != 0) & (fault != VAC) & (term == self.term),
        }
        for k, x in tests.items():
            if x.any():
                self.kinds.add(k)
        self.self_only += int((tests["became leader"] & (cb == (1 << cur["self_slot"]))).sum())
        self.left |= np.where(pl & cl, left, 0).astype(np.uint8)
        self.closed = (self.closed | (fault == VAC)) & ~cl
        self.term = term

    def check(self, what="", ref=None, vacant=None, census=True):
        """a watch of the whole engine returns exactly the pending slots, ascending, as their current view - which is
        ref's; a second watch returns nothing; the census is numpy's"""
        cur, m = self.expect()
        if ref is not None:
            want = view_of(ref, self.seen, self.leave, self.join, vacant=vacant)
            assert cur.tobytes() == want.tobytes(), (what, np.nonzero(key_of(cur) != key_of(want))[0][:8])
        rows, total = self.watch()
        assert total == int(m.sum()), (what, total, int(m.sum()))
        assert rows.tobytes() == cur[m].tobytes(), (what, rows[:4], cur[m][:4])
        self.classify(cur, m)
        self.seen = key_of(cur)
        rows, total = self.watch()
        assert total == 0 and len(rows) == 0, what
        if census:
            G = self.e.G
            check_census(self.e, what, limits=(0, self.leave, U64_MAX), cuts=[(0, G), (G // 3, G // 2)])
        return int(m.sum())


def elect(engines, gs, now_ms):
    """Timeout + granted votes at the term the Timeout reaches, for the slots gs, on every engine alike"""
    gs = np.asarray(gs, np.uint32)
    for e in engines:
        e.submit_columns(np.full(len(gs), capi.CMD_TIMEOUT, np.uint8), gs)
        e.step(now_ms)
        slots, term = e.read("self_slot")[gs].astype(np.int64), e.read("term")[gs].astype(np.uint64)
        ids = np.array(e.node_ids, np.uint32)
        for k in range(1, e.R // 2 + 1):
            e.submit_columns(np.full(len(gs), capi.CMD_VOTE_RESPONSE, np.uint8), gs, from_=ids[(slots + k) % e.R], term=term,
                             flag=np.ones(len(gs), np.uint8))
            e.step(now_ms)
        drain_all(e)
        assert (e.read("role")[gs] == capi.ROLE_LEADER).all()


def dense_tick(engines, appends, ack):
    """one dense tick on every engine alike: every healthy leader appends `appends` blocks; ack(r, head, slot) -> the [G] ack
    heads of the members at distance r = 1 .. R - 1 behind the own slot (NO_ACK: silent)"""
    e0 = engines[0]
    G, R = e0.G, e0.R
    leads, head, _, slot = lags_of(e0, 0, G)
    acks = np.full((R, G), capi.NO_ACK, np.uint64)
    gs = np.nonzero(leads)[0]
    acks[slot[gs].astype(np.int64), gs] = appends
    for k in range(1, R):
        a = np.asarray(ack(k, head, slot), np.uint64)
        acks[(slot[gs].astype(np.int64) + k) % R, gs] = np.broadcast_to(a, (G,))[gs]
    for e in engines:
        e.step_dense_acks(acks)
        drain_all(e)


# ---- 1. every kind of transition, exact ------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,seed", [pytest.param(96, 3, 1, id="small-3"), pytest.param(80, 5, 2, id="small-5")])
def test_every_kind_of_transition(G, R, seed):
    rng = np.random.default_rng(seed)
    slots = rng.integers(0, R, G).astype(np.uint8)
    e, kw = fresh(G, R, R + seed, slots)
    ref = RefEngine(G, R, **kw)
    both = (e, ref)
    feed = Feed(e, leave=4, join=1)
    assert feed.check("fresh", ref) == 0  # a fresh engine reports nothing until something leads
    lead = np.arange(G) % 2 == 0
    gs = np.nonzero(lead)[0]
    elect(both, gs, 10)
    assert feed.check("elected", ref) == len(gs)
    everybody = lambda k, head, slot: head  # noqa: E731
    for t in range(2):
        dense_tick(both, 3, everybody)
        feed.check(f"all ack {t}", ref)
    assert (feed.seen[gs] == (SEEN_LEADS | ((1 << R) - 1))).all()
    for t in range(3):  # the member behind the own slot goes silent: it leaves above leave_lag
        dense_tick(both, 3, lambda k, head, slot: np.where(k == 1, capi.NO_ACK, head).astype(np.uint64))
        feed.check(f"one silent {t}", ref)
    assert "follower left" in feed.kinds and "went below quorum" not in feed.kinds
    assert (popcount8(feed.seen[gs] & 0xff) == R - 1).all()
    for t in range(3):  # everybody silent: the sets shrink to {self}, below quorum
        dense_tick(both, 3, lambda k, head, slot: capi.NO_ACK)
        feed.check(f"all silent {t}", ref)
    assert "went below quorum" in feed.kinds and (popcount8(feed.seen[gs] & 0xff) == 1).all()
    dense_tick(both, 3, everybody)  # (the acks of a tick are those of the head before its appends: lag 3 > join_lag)
    dense_tick(both, 0, everybody)
    feed.check("everybody back", ref)
    assert "follower rejoined" in feed.kinds and (feed.seen[gs] == (SEEN_LEADS | ((1 << R) - 1))).all()
    # a forged ack ABOVE the head counts as caught up: no row
    forged = gs[::3]
    dense_tick(both, 0, lambda k, head, slot: np.where(np.isin(np.arange(G), forged) & (k == 1), head + 50, head).astype(np.uint64))
    ok = e.read("fault")[forged] == 0
    assert ok.any()  # (the scenario exists: a forged ack that is stored above the head, on a slot that goes on leading)
    k1 = (slots[forged].astype(np.int64) + 1) % R
    m1 = np.array([e.read("match", int(r), int(g), 1)[0] for r, g in zip(k1, forged)])
    assert (m1[ok] > e.read("head")[forged][ok]).all()
    before = feed.seen.copy()
    feed.check("forged ack", ref)
    assert (feed.seen[forged][ok] == before[forged][ok]).all()
    # an AppendEntries of a higher term from another member (leader.rs:200-204): the leaders among the first quarter meet
    # term 7 - where the reference's process dies (leader.rs:33-35), so the slot stops leading at that term
    down = gs[gs < G // 4]
    ids = np.array(e.node_ids, np.uint32)
    for x in both:
        x.submit_columns(np.full(len(down), capi.CMD_APPEND_ENTRIES, np.uint8), down.astype(np.uint32),
                         from_=ids[(slots[down].astype(np.int64) + 1) % R], term=np.full(len(down), 7, np.uint64),
                         id=np.zeros(len(down), np.uint64), aux=np.zeros(len(down), np.uint64))
        x.step(400)
        drain_all(x)
    assert (e.read("term")[down] == 7).all() and (e.read("role")[down] == capi.ROLE_LEADER).all()
    assert feed.check("higher term", ref) == int((before[down] & SEEN_LEADS != 0).sum()) >= 1
    assert "lost leadership to a higher term" in feed.kinds and "faulted" not in feed.kinds
    # ... the process restarts on its tree and is elected again: its members' progress starts over, the set is {self}
    for x in both:
        x.submit_columns(np.full(len(down), capi.CMD_RESTART, np.uint8), down.astype(np.uint32))
        x.step(1000)
        drain_all(x)
    assert feed.check("restarted", ref) == 0
    elect(both, down, 2000)
    feed.check("elected again", ref)
    assert feed.self_only > 0
    dense_tick(both, 0, everybody)
    feed.check("acks after the second election", ref)
    # an AppendResponse from a node the leader's progress does not know (progress.rs:43): a reference-domain fault
    bad = gs[(gs >= G // 4) & (gs < G // 2)][:5].astype(np.uint32)
    for x in both:
        x.submit_columns(np.full(len(bad), capi.CMD_APPEND_RESPONSE, np.uint8), bad, from_=np.full(len(bad), 77, np.uint32),
                         term=x.read("term")[bad].astype(np.uint64), id=np.ones(len(bad), np.uint64), flag=np.ones(len(bad), np.uint8))
        x.step(2100)
        drain_all(x)
    assert (e.read("fault")[bad] != 0).all()
    assert feed.check("faulted", ref) == len(bad) and "faulted" in feed.kinds
    # close led slots (ref_py knows no vacancy: its copies go on, masked), open them again, elect them (the engine alone)
    shut = gs[gs >= 3 * G // 4]
    e.close_groups(shut)
    assert feed.check("closed", ref, vacant=shut) == len(shut) and "closed" in feed.kinds
    e.open_groups(shut, 3000)
    assert feed.check("opened: followers at term 0") == 0
    elect((e,), shut, 3100)
    assert feed.check("opened and elected") == len(shut)
    assert feed.kinds == set(KINDS), sorted(set(KINDS) - feed.kinds)


# ---- 2. one follower down, then back: the stream of test_follower_down_stays_on_the_fast_path_and_exact -------------------
@pytest.mark.parametrize("R,leave", [pytest.param(3, 100, id="small-3-below-the-field-limit"),
                                     pytest.param(3, 70000, id="small-3-above-the-field-limit"),
                                     pytest.param(5, 100, id="small-5-below-the-field-limit"),
                                     pytest.param(5, 2000, id="small-5-above-the-field-limit")])
def test_follower_down_then_back(R, leave):
    """R = 5: a lag field holds up to 1021, R = 3 up to 65533.  With leave_lag below that a BEHIND field is "out" without
    the wide column; at or above it the wide column decides - the down follower leaves later, when its real lag passes
    leave_lag."""
    from josefine_amd.traces import elect_all
    G = 48
    kw = dict(seed=41, flags=capi.CFG_SEPARATE_COMMIT_KEY)
    # (ref_py appends block by block in Python: at R = 3 - a thousand appends per tick and slot - the engine's own columns
    # alone state the view)
    e, ref = BatchedRaft(G, R, **kw), (RefEngine(G, R, **kw) if R == 5 else None)
    both = (e,) if ref is None else (e, ref)
    for x in both:
        elect_all(x)
        drain_all(x)
    esc = (1 << (64 // (R + 1))) - 1
    assert (leave >= esc - 1) == (leave in (70000, 2000))
    feed = Feed(e, leave, leave // 2)
    feed.check("elected", ref)
    per = max(1, esc // 60)  # appends per tick: ~70 ticks to leave a field
    T_quorum, T_back = 160, 240
    rng = np.random.default_rng(7)
    left_at = None
    for t in range(T_back + 6):
        acks = np.full((R, G), capi.NO_ACK, np.uint64)
        head = e.read("head").astype(np.uint64)
        acks[0, :] = per + (rng.integers(0, 2, G) if t % 5 == 0 else 0)
        up = list(range(1, R))
        if t < T_back:
            up = [r for r in up if r != 1]          # slot 1 is down from the start
        if T_quorum <= t < T_back:
            up = [r for r in up if r > R // 2 + 1]  # ... then more than a minority
        for r in up:
            acks[r, :] = head
        if t >= T_back:
            acks[1, ::2] = head[::2] // 2           # the returning follower catches up in steps
        for x in both:
            x.step_dense_acks(acks)
            drain_all(x)
        feed.check(f"tick {t}", ref, census=t % 16 == 0 or t >= T_back - 2)
        if left_at is None and not (feed.seen[0] >> 1) & 1:
            left_at = t
    assert not e.read("fault").any() and (e.read("head") > 2 * esc).all()
    # slot 1 left when its lag passed leave_lag: about leave / per ticks in
    assert left_at is not None and abs(left_at - leave // per) <= 2, (left_at, leave // per)
    assert "follower left" in feed.kinds
    # the others are silent for T_back - T_quorum ticks: they leave too where that many appends pass leave_lag
    assert ("went below quorum" in feed.kinds) == ((T_back - T_quorum) * per > leave)
    # everybody acknowledges the head: whole sets again
    for t in range(2):
        head = e.read("head").astype(np.uint64)
        acks = np.broadcast_to(head, (R, G)).copy()
        acks[0, :] = 0
        for x in both:
            x.step_dense_acks(acks)
            drain_all(x)
        feed.check(f"back {t}", ref)
    assert (feed.seen == (SEEN_LEADS | ((1 << R) - 1))).all() and "follower rejoined" in feed.kinds


# ---- 3. hysteresis ------------------------------------------------------------------------------------------------------
LAGS = (1, 2, 3, 4, 5, 6, 7, 6, 4, 5, 4, 3, 4, 5, 6, 5)  # (a progress head never goes back: a lag grows by the appends at most)


def rows_expected(lags, leave, join, G):
    """the rows a feed owes a stream of lags of one member, by the rule alone: in -> out above leave, out -> in at join"""
    out, inside = [], True
    for L in lags:
        now = L <= (leave if inside else join)
        out.append(G if now != inside else 0)
        inside = now
    return out


@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_hysteresis(R):
    G = 64
    slots = (np.arange(G) % R).astype(np.uint8)
    for leave, join, with_ref in ((6, 3, True), (4, 4, False)):
        e = BatchedRaft(G, R, seed=3, self_slots=slots)
        both = (e, RefEngine(G, R, seed=3, self_slots=slots)) if with_ref else (e,)
        ref = both[-1] if with_ref else None
        elect(both, np.arange(G), 10)
        feed = Feed(e, leave, join)
        dense_tick(both, 3, lambda k, head, slot: head)
        dense_tick(both, 0, lambda k, head, slot: head)
        feed.check("in sync", ref)
        totals = []
        for L in LAGS:  # one append a tick; the member behind the own slot acknowledges `head - L` of the new head
            dense_tick(both, 1, lambda k, head, slot: (head + 1 - np.where(k == 1, L, 1)).astype(np.uint64))
            _, _, lag, _ = lags_of(e, 0, G)
            assert (lag.max(axis=0) == L).all(), (L, lag.max(axis=0)[:4])
            totals.append(feed.check(f"lag {L}", ref))
        assert totals == rows_expected(LAGS, leave, join, G), (leave, join, totals)
        if join < leave:
            # between join_lag and leave_lag nothing is reported, in either direction: it left at 7 and came back at 3
            assert [L for L, n in zip(LAGS, totals) if n] == [7, 3]
        else:
            assert sum(1 for n in totals if n) == 5  # without hysteresis the same stream crosses the one threshold five times
        assert {"follower left", "follower rejoined"} <= feed.kinds


# ---- 4. a restarted and re-elected leader: the lags' base is the run's top ------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_restarted_leader(R):
    G = 64
    slots = (np.arange(G) % R).astype(np.uint8)
    e, kw = fresh(G, R, 5, slots)
    ref = RefEngine(G, R, **kw)
    both = (e, ref)
    elect(both, np.arange(G), 10)
    feed = Feed(e, 4, 1)
    dense_tick(both, 5, lambda k, head, slot: head)
    dense_tick(both, 0, lambda k, head, slot: head)   # committed: 5
    dense_tick(both, 6, lambda k, head, slot: capi.NO_ACK)  # 6 more that nobody acknowledges
    feed.check("before", ref)
    top = e.read("head").copy()
    for x in both:
        x.apply_all(Command.Restart(), 3000)
        drain_all(x)
    assert feed.check("restarted", ref) == G  # nobody leads
    assert (e.read("head") < top).all()  # the head is back at the commit index, the run above it still there
    elect(both, np.arange(G), 4000)
    feed.check("elected again", ref)
    assert feed.self_only > 0
    # acks between the head and the run's top count as caught up; acks below the head are lags
    ids = np.array(e.node_ids, np.uint32)
    term = e.read("term").astype(np.uint64)
    head = e.read("head").astype(np.uint64)
    for k, ack in ((1, top.astype(np.uint64)), (2, head - 2)):
        for x in both:
            x.submit_columns(np.full(G, capi.CMD_APPEND_RESPONSE, np.uint8), np.arange(G, dtype=np.uint32),
                             from_=ids[(slots.astype(np.int64) + k) % R], term=term, id=ack, flag=np.ones(G, np.uint8))
            x.step(4100)
            drain_all(x)
        feed.check(f"ack {k}", ref)
    assert not e.read("fault").any()
    got = feed.seen & 0xff
    assert (((got >> ((slots.astype(np.int64) + 1) % R)) & 1) == 1).all()  # the top's ack: in sync
    check_census(e, "restarted leaders")


# ---- 5. acks through the general state machine and jg_step_node; watching changes nothing --------------------------------
def same_drains(a, b, ref, what):
    for fn in DRAINS:
        want = getattr(ref, fn)()
        for e in (a, b):
            got = getattr(e, fn)()
            assert got.tobytes() == want.tobytes(), (what, fn, len(got), len(want))


@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_fuzz_and_watching_changes_nothing(R):
    G = 96
    rng = np.random.default_rng(11 + R)
    slots = rng.integers(0, R, G).astype(np.uint8)
    a, kw = fresh(G, R, 5, slots)
    b, _ = fresh(G, R, 5, slots)
    ref = RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    for x in (a, b, ref):
        elect((x,), np.arange(G), 10)
    feed = Feed(a, 2, 0)

    def look(what, r=None):
        feed.check(what, r)
        feed.watch(g0=10, n=50, limit=3, peek=True)
        a.replication_census(1, 7, 80)

    look("elected", ref)
    now, changed = 10, 0
    for s in range(16):  # the general state machine, against the twin and ref_py
        batch = random_batch(rng, ref, 3 * G, foreign_voters=True, budget=budget)
        now += int(rng.integers(0, 300))
        for e in (a, b, ref):
            e.submit_columns(**batch)
            e.step(now)
        look(f"step {s}", ref)
        same_drains(a, b, ref, f"step {s}")
        compare_snapshots(a, ref, f"step {s}")
    for t in range(4):  # dense ticks
        leads, head, _, slot = lags_of(ref, 0, G)
        acks = np.full((R, G), capi.NO_ACK, np.uint64)
        gs = np.nonzero(leads & (rng.random(G) < 0.7))[0]
        acks[slot[gs].astype(np.int64), gs] = 3
        acks[(slot[gs].astype(np.int64) + 1) % R, gs] = head[gs]
        for e in (a, b, ref):
            e.step_dense_acks(acks)
        look(f"dense {t}", ref)
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
    assert {"follower joined", "follower left"} <= feed.kinds, feed.kinds


# ---- 6. limit and peek, ranges off the tile boundaries, a G that is no multiple of the tile -------------------------------
@pytest.mark.parametrize("limit", [pytest.param(61, id="small-61"), pytest.param(500, id="small-500")])
def test_limit_and_peek(limit):
    from josefine_amd.traces import elect_all
    G, R = ISR_TILE + 300, 3
    e = BatchedRaft(G, R, seed=3, self_slots=(np.arange(G) % R).astype(np.uint8))
    feed = Feed(e, 4, 1)
    elect_all(e, 10)
    drain_all(e)
    cur, m = feed.expect()
    pending = int(m.sum())
    assert pending == G
    for _ in range(2):  # a peek delivers the same rows and advances nothing
        rows, total = feed.watch(limit=limit, peek=True)
        assert total == pending and rows.tobytes() == cur[m][:limit].tobytes()
    for g0, n in ((ISR_TILE - 3, 7), (1, ISR_TILE), (255, 258), (G - 1, 1), (5, 0)):
        rows, total = feed.watch(g0=g0, n=n, peek=True)
        assert total == n and rows.tobytes() == cur[g0:g0 + n].tobytes(), (g0, n)
    rows, total = feed.watch(g0=ISR_TILE - 3, n=7)  # a range across the tile border is delivered, and only it
    assert total == 7
    feed.seen[rows["group"]] = key_of(rows)
    pending -= 7
    got = [rows]
    while pending:
        rows, total = feed.watch(limit=limit)
        assert total == pending and len(rows) == min(limit, pending)
        cur, m = feed.expect()
        assert rows.tobytes() == cur[m][:limit].tobytes()
        feed.seen[rows["group"]] = key_of(rows)
        got.append(rows)
        pending -= len(rows)
    allrows = np.concatenate(got[1:])
    assert (np.diff(allrows["group"].astype(np.int64)) > 0).all()  # ascending over the calls: nothing lost, nothing twice
    assert np.bincount(np.concatenate(got)["group"], minlength=G).tolist() == [1] * G
    assert feed.watch()[1] == 0 and feed.watch(limit=0)[1] == 0


# ---- 7. the control plane, seen through the diff alone -------------------------------------------------------------------
def test_small_control_plane():
    G, R = 192, 3
    src = BatchedRaft(G, R, seed=2)
    dst = BatchedRaft(G, R, seed=2, start_vacant=True)
    fs, fd = Feed(src, 4, 1), Feed(dst, 4, 1)
    assert fs.check("fresh") == 0 and fd.check("start vacant") == 0
    elect((src,), np.arange(96), 10)  # slots 0 .. 95 lead
    assert fs.check("elected") == 96
    src.close_groups(range(0, 10))
    rows, total = fs.watch(peek=True)
    assert total == 10 and rows["group"].tolist() == list(range(10)) and (rows["state"] == 0).all() and (rows["isr"] == 0).all()
    assert (rows["head"] == 0).all() and (rows["worst_lag"] == 0).all() and (rows["replicate"] == 0).all()
    assert fs.check("closed") == 10 and "closed" in fs.kinds
    # a move of leaders and followers: the destination reports the leaders, the source reports them gone
    move_groups(src, dst, 80, 30, close_source=True)
    rows, total = fd.watch(peek=True)
    assert total == 16 and rows["group"].tolist() == list(range(80, 96)) and ((rows["state"] & LEADS) != 0).all()
    assert fd.check("imported") == 16
    rows, total = fs.watch(peek=True)
    assert total == 16 and rows["group"].tolist() == list(range(80, 96)) and (rows["state"] == 0).all()
    assert fs.check("moved away") == 16
    assert (src.read("fault")[80:110] == VAC).all()
    dst.open_groups(range(150, 160), 500)
    assert fd.check("opened: followers") == 0
    check_census(src, "source")
    check_census(dst, "destination")


# ---- 8. the census ---------------------------------------------------------------------------------------------------------
def test_small_census():
    G, R = 4096 + 300, 5
    rng = np.random.default_rng(9)
    slots = rng.integers(0, R, G).astype(np.uint8)
    e = BatchedRaft(G, R, seed=4, self_slots=slots)
    cuts = [(0, G), (1, G - 1), (3, 0), (G - 5, 5), (G // 3, G // 2), (0, 1024), (7, 1023), (5, 1025), (1021, 7)]
    check_census(e, "no leader at all", cuts=cuts)
    c = e.replication_census(0)
    assert c["leaders"] == 0 and c["max_uncommitted"] == 0 and not any(c["max_lag"]) and not any(c["out_of_sync"])
    lead = rng.random(G) < 0.5
    elect((e,), np.nonzero(lead)[0], 10)
    check_census(e, "elected", cuts=cuts)
    dense_tick((e,), 7, lambda k, head, slot: head)
    # ragged lags; one member 1100 behind - at R = 5 outside its 10-bit field - and one forged above the head
    none = np.uint64(capi.NO_ACK)
    some = lambda hi, on: rng.integers(0, hi, G).astype(np.uint64) * np.uint64(on)  # noqa: E731
    dense_tick((e,), 1100, lambda k, head, slot: np.where(k == 1, none, head + some(9, k == 2)))
    dense_tick((e,), 4, lambda k, head, slot: np.where(k == 1, none, head - some(5, k != 3)))
    c = e.replication_census(20)
    assert c["leaders"] == int((lead & (e.read("fault") == 0)).sum()) and max(c["max_lag"]) >= 1100 and c["under_replicated"] > 0
    check_census(e, "lagging", limits=(0, 3, 1000, 1104, 1 << 40, U64_MAX), cuts=cuts)
    e.close_groups(np.sort(rng.choice(G, G // 5, replace=False)))
    check_census(e, "vacant", cuts=cuts)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------
def test_small_refusals():
    G, R = 200, 3
    e, twin = BatchedRaft(G, R, seed=4), BatchedRaft(G, R, seed=4)
    for x in (e, twin):
        elect((x,), np.arange(50), 10)
    api, h = e.api, e._h
    rows = np.zeros(G, capi.ISR_ROW_DTYPE)
    total, c = C.c_size_t(0), capi.ReplCensus()
    pol, bad = capi.IsrPolicy(4, 1), capi.IsrPolicy(1, 4)
    watch = lambda flags, p, g0, n, out, cap, tot: api.engine_watch_replicas(h, flags, p, g0, n, out, cap, tot)  # noqa: E731
    P = C.byref(pol)
    assert watch(0, P, 0, G, rows.ctypes.data, G, None) == capi.EINVAL            # a null total
    assert watch(0, P, 0, G, None, 5, C.byref(total)) == capi.EINVAL              # a null out with cap > 0
    assert watch(2, P, 0, G, rows.ctypes.data, G, C.byref(total)) == capi.EINVAL  # an unknown flag
    assert watch(0, P, G - 1, 2, rows.ctypes.data, G, C.byref(total)) == capi.EINVAL
    assert watch(0, P, 1, 0xFFFFFFFF, rows.ctypes.data, G, C.byref(total)) == capi.EINVAL
    assert watch(0, None, 0, G, rows.ctypes.data, G, C.byref(total)) == capi.EINVAL           # a null policy
    assert watch(0, C.byref(bad), 0, G, rows.ctypes.data, G, C.byref(total)) == capi.EINVAL   # join_lag > leave_lag
    assert api.engine_watch_replicas(None, 0, P, 0, G, rows.ctypes.data, G, C.byref(total)) == capi.EINVAL
    assert api.engine_replication_census(h, 0, 0, G, None) == capi.EINVAL
    assert api.engine_replication_census(h, 0, G, 1, C.byref(c)) == capi.EINVAL
    assert api.engine_replication_census(None, 0, 0, G, C.byref(c)) == capi.EINVAL
    with pytest.raises(EngineError):
        e.watch_replicas(1, 4)
    assert watch(capi.WATCH_PEEK, P, 0, G, None, 0, C.byref(total)) == capi.OK and total.value == 50  # nothing was advanced
    # kept node steps outstanding: refused with read_chains's code, and the kept steps are still viewable afterwards
    for x in (e, twin):
        x.step_node_begin(1000, async_=True, keep=True)
        x.step_node_begin(1100, async_=True, keep=True)
    r = capi.ChainRead()
    r.n, off = G, np.zeros(G + 1, np.uint64)
    r.off = off.ctypes.data
    code = api.engine_read_chains(h, C.byref(r), C.byref(C.c_uint64(0)))
    assert code == capi.EINVAL
    assert watch(0, P, 0, G, rows.ctypes.data, G, C.byref(total)) == code and api.engine_replication_census(h, 0, 0, G, C.byref(c)) == code
    with pytest.raises(EngineError):
        e.watch_replicas(4)
    outs = [[x.node_outbox(), x.node_outbox()] for x in (e, twin)]
    for k in range(2):
        for name, v in outs[0][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][k][name])), (k, name)
    compare_drains(e, twin, "kept")
    compare_snapshots(e, twin, "kept")
    assert e.watch_replicas(4, 1)[1] == 50 and e.replication_census(4) == census_np(e, 4)


# ---- 10. shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [pytest.param(2, id="small-2-shards"), pytest.param(3, id="small-3-shards")])
def test_shards(D):
    G, R = 1000, 3
    rng = np.random.default_rng(D)
    s = BatchedRaft(G, R, seed=4, device_ids=[0] * D)
    one = BatchedRaft(G, R, seed=4)
    last, first = s.shard(D - 1).group_lo, s.shard(0).G

    def same(what, **kw):
        a, b = s.watch_replicas(4, 1, **kw), one.watch_replicas(4, 1, **kw)
        assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes(), (what, kw, a[1], b[1])
        return a

    assert same("fresh")[1] == 0
    for e in (s, one):
        elect((e,), np.arange(G), 10)
    same("count", limit=0)
    same("a range across the shard border", g0=first - 5, n=11, peek=True)
    rows, total = same("a limit that ends inside the first shard", limit=first // 2)
    assert total == G and rows["group"].tolist() == list(range(first // 2))
    rows, total = same("peek", peek=True, limit=7)
    assert total == G - first // 2 and rows["group"][0] == first // 2  # the shards behind the limit kept their shadows
    rows, total = same("the rest")
    assert total == G - first // 2 and rows["group"][0] == first // 2 and rows["group"][-1] == G - 1
    assert same("quiet")[1] == 0
    for e in (s, one):
        dense_tick((e,), 6, lambda k, head, slot: np.where((np.arange(G) % 3 == 0) & (k == 1), capi.NO_ACK, head).astype(np.uint64))
        dense_tick((e,), 6, lambda k, head, slot: np.where((np.arange(G) % 3 == 0) & (k == 1), capi.NO_ACK, head).astype(np.uint64))
        e.close_groups(np.sort(np.random.default_rng(5).choice(G, 100, replace=False)))
    for g0, n in ((0, G), (1, last + 3), (last - 2, 7), (G - 1, 1), (0, 0)):
        for limit in (0, 6, U64_MAX):
            assert s.replication_census(limit, g0, n) == one.replication_census(limit, g0, n) == census_np(one, limit, g0, n), (g0, n, limit)
    same("a limit of 1", limit=1)
    same("the last shard alone", g0=last, n=G - last, limit=3)
    rows, total = same("the rest")
    assert total > 100 and (np.diff(rows["group"].astype(np.int64)) > 0).all()
    assert same("quiet")[1] == 0
    compare_snapshots(s, one, "shards")


# ---- 11. full size (the device only) -----------------------------------------------------------------------------------------
def test_one_percent_of_the_followers_down_1m():
    from josefine_amd.traces import elect_all
    G, R = 1 << 20, 5
    rng = np.random.default_rng(6)
    e = BatchedRaft(G, R, seed=5, self_slots=(np.arange(G) % R).astype(np.uint8))
    elect_all(e, 10)
    drain_all(e)
    feed = Feed(e, 4, 1)
    assert feed.check("elected", census=False) == G
    down = rng.random((R, G)) < 0.01  # (distance behind the own slot, slot): about 1 % of the followers
    dense_tick((e,), 3, lambda k, head, slot: head)
    dense_tick((e,), 0, lambda k, head, slot: head)
    feed.check("in sync", census=False)
    assert (feed.seen == (SEEN_LEADS | 31)).all()
    for t in range(3):
        dense_tick((e,), 3, lambda k, head, slot: np.where(down[k], capi.NO_ACK, head).astype(np.uint64))
        n = feed.check(f"down {t}", census=False)
        print(f"tick {t}: {n} rows")
    want = int(down[1:].any(axis=0).sum())
    assert int((popcount8(feed.seen & 0xff) < R).sum()) == want and want > G // 50
    for limit in (0, 4, U64_MAX):
        assert e.replication_census(limit) == census_np(e, limit), limit
    dense_tick((e,), 0, lambda k, head, slot: head)
    assert feed.check("back", census=False) == want and "follower rejoined" in feed.kinds
    assert feed.watch(limit=0)[1] == 0
