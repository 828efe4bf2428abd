"""The commit feed (ABI v17): jg_engine_watch_commits - which partitions' commit index or head moved since the feed last
delivered them, and from where to where: the fsm_tx the dense entry points do not queue.  The commit view of a slot is
(commit, head) as jg_read_state returns them, so the expected rows are stated in numpy over the engine's own read(...)
columns and a `seen` array of (commit, head) as last delivered: a watch returns exactly the slots that differ, ascending,
every field equal; the backlog equals the numpy counts and sums; nothing a step, a drain, a read or the other feeds can
observe changes.  Cases whose id contains "small" are small enough for the emulated device
(tests/test_commit_feed_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, DenseCluster, capi, commit_rows_as_fsm, expand_fsm_rows, move_groups
from josefine_amd.engine import EngineError
from fuzz import random_batch
from parity import compare_drains, compare_snapshots
from test_lookup_groups import tick, world
from test_move_groups import drain_all
from test_replica_feed import dense_tick, elect
from test_vacant_groups import DRAINS, fresh

pytestmark = pytest.mark.gpu

VAC = capi.FAULT_VACANT
COMMITTED, APPENDED, REWOUND = capi.CMT_COMMITTED, capi.CMT_APPENDED, capi.CMT_REWOUND
LEADS, VACANT, FAULTED = capi.CMT_LEADS, capi.CMT_VACANT, capi.CMT_FAULTED
TILE = 256 * 4  # slots per tile of the watch passes (jg_commits.h JG_CMT_TILE)
GC = 2 * TILE + 37  # the compaction cases: a ragged last tile
BACKLOG = [name for name, _ in capi.CommitBacklog._fields_]


def view_of(e, seen, g0=0, n=None):
    """the commit view of slots g0 .. g0 + n - 1 from e.read(...) against `seen` ([G, 2]: commit, head as last delivered), as
    rows - of every slot, differing or not"""
    n = e.G - g0 if n is None else n
    v = np.zeros(n, capi.COMMIT_ROW_DTYPE)
    if not n:
        return v
    rd = lambda k: e.read(k, 0, g0, n)  # noqa: E731
    role, fault = rd("role"), rd("fault")
    c, h = rd("commit").astype(np.uint64), rd("head").astype(np.uint64)
    cf, hf = seen[g0:g0 + n, 0], seen[g0:g0 + n, 1]
    v["group"], v["role"], v["fault"], v["self_slot"], v["term"] = g0 + np.arange(n), role, fault, rd("self_slot"), rd("term")
    v["commit_from"], v["commit"], v["head_from"], v["head"] = cf, c, hf, h
    v["state"] = (np.where(c > cf, COMMITTED, 0) | np.where(h > hf, APPENDED, 0) | np.where((c < cf) | (h < hf), REWOUND, 0) |
                  np.where((role == capi.ROLE_LEADER) & (fault == 0), LEADS, 0) | np.where(fault == VAC, VACANT, 0) |
                  np.where((fault != 0) & (fault != VAC), FAULTED, 0))
    return v


def differs(v, commits_only=False):
    m = v["commit"] != v["commit_from"]
    return m if commits_only else m | (v["head"] != v["head_from"])


def backlog_np(v, m):
    r = v[m]
    up_c, up_h = r["commit"] > r["commit_from"], r["head"] > r["head_from"]
    down = (r["commit"] < r["commit_from"]) | (r["head"] < r["head_from"])
    return dict(changed=len(r), committed=int(up_c.sum()), appended=int(up_h.sum()), rewound=int(down.sum()),
                pending_commits=int(np.sum((r["commit"] - r["commit_from"])[up_c], dtype=np.uint64)),
                pending_appends=int(np.sum((r["head"] - r["head_from"])[up_h], dtype=np.uint64)))


def same(got, want, what=""):
    if got.tobytes() != want.tobytes():
        assert len(got) == len(want), (what, len(got), len(want))
        for k in got.dtype.names:
            bad = np.nonzero(got[k] != want[k])[0]
            assert not len(bad), (what, k, bad[:6], got[k][bad[:6]], want[k][bad[:6]])
    assert got.tobytes() == want.tobytes(), what


class Feed:
    """the test's statement of one engine's feed: `seen` is the (commit, head) the watch last delivered per slot"""

    def __init__(self, e):
        self.e, self.seen = e, np.zeros((e.G, 2), np.uint64)

    def advance(self, rows):
        self.seen[rows["group"], 0], self.seen[rows["group"], 1] = rows["commit"], rows["head"]

    def poll(self, what="", g0=0, n=None, limit=None, peek=False, commits_only=False):
        """one watch, held to numpy: the total, the rows (the first `limit` of the slots that differ, ascending, every field
        equal), the backlog; the delivered rows become seen unless peeking.  Returns the rows."""
        n = self.e.G - g0 if n is None else n
        cur = view_of(self.e, self.seen, g0, n)
        m = differs(cur, commits_only)
        want = cur[m] if limit is None else cur[m][:limit]
        rows, total, b = self.e.watch_commits(g0, n, limit, peek, commits_only, backlog=True)
        assert total == int(m.sum()), (what, total, int(m.sum()))
        same(rows, want, what)
        assert b == backlog_np(cur, m), (what, b, backlog_np(cur, m))
        assert b["changed"] == total
        if not peek:
            self.advance(rows)
        return rows

    def settle(self, what=""):
        """everything pending is delivered; the feed is then silent"""
        rows = self.poll(what)
        assert self.e.watch_commits()[1] == 0 and self.e.watch_commits(limit=0, commits_only=True)[1] == 0, what
        return rows


def has(rows, gs, bits, none=0):
    """every slot of gs has a row, with all of `bits` and none of `none` in its state"""
    r = rows[np.isin(rows["group"], gs)]
    return len(r) == len(gs) and len(gs) > 0 and ((r["state"] & bits) == bits).all() and not (r["state"] & none).any()


# ---- 1. every decode branch, from a zero shadow ----------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(5, id="small-5"), pytest.param(3, id="small-3")])
def test_every_decode_branch(R):
    w = world(R)  # (test_lookup_groups: 300 slots in every state the decode of a leader's commit distinguishes)
    feed = Feed(w.e)
    rows = feed.poll("the world", peek=True)
    among = np.zeros(w.G, bool)
    among[rows["group"]] = True
    for k in ("a leader wholly in lag space", "a leader with a BEHIND field", "a leader with an ABOVE field", "a leader whose base is run_hi",
              "a leader whose commit is in the wide column", "a follower that knows a leader and has voted",
              "a faulted slot"):
        assert (w.states[k] & among).any(), k  # a condition of the test: the state is among the rows compared
    assert ((rows["state"] & LEADS) != 0).any() and ((rows["state"] & FAULTED) != 0).any()
    assert not among[w.states["a vacant slot"]].any()  # a vacant slot's view is (0, 0): nothing against a zero shadow
    for g0, n in ((1, w.G - 1), (3, 0), (w.G - 5, 5), (100, 60)):
        feed.poll("a range", g0=g0, n=n, peek=True)
        feed.poll("a range, commits only", g0=g0, n=n, peek=True, commits_only=True)
    rows = feed.poll("commits only", commits_only=True)
    assert len(rows) and (rows["commit"] != 0).all()
    feed.settle("the rest: the slots whose head alone moved")


# ---- 2. every state bit: the scenario ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,seed", [pytest.param(3, 1, id="small-3"), pytest.param(5, 2, id="small-5")])
def test_every_kind_of_transition(R, seed):
    G = 96
    rng = np.random.default_rng(seed)
    slots = rng.integers(0, R, G).astype(np.uint8)
    e, _ = fresh(G, R, R + seed, slots)
    ids = np.array(e.node_ids, np.uint32)
    feed = Feed(e)
    assert len(feed.settle("fresh")) == 0  # a fresh engine reports nothing until something is appended or committed
    sv = BatchedRaft(G, R, seed=3, start_vacant=True)
    assert len(Feed(sv).settle("start vacant")) == 0
    at = np.arange(G)
    gs, fs = at[at % 2 == 0], at[at % 2 == 1]  # the even slots lead, the odd ones follow
    elect((e,), gs, 10)
    feed.settle("elected")
    everybody = lambda k: e.read("head")  # noqa: E731
    # a leader committing: three appends, acknowledged a tick later
    tick(e, 3, everybody)
    rows = feed.settle("appended")
    assert has(rows, gs, LEADS | APPENDED, REWOUND)
    tick(e, 0, everybody)
    rows = feed.settle("committed")
    assert has(rows, gs, LEADS | COMMITTED, REWOUND | APPENDED) and (rows["commit"] == 3).all() and (rows["commit_from"] == 0).all()
    # the commit field escapes to the wide column: close to 2^20 appends a tick nobody acknowledges, for a few ticks
    wide = gs[:6]
    for t in range(3):
        tick(e, np.where(np.isin(at, wide), capi.MAX_DENSE_APPENDS - 3, 0), lambda k: capi.NO_ACK)
        rows = feed.settle(f"unacknowledged {t}")
        assert has(rows, wide, LEADS | APPENDED, COMMITTED) and len(rows) == len(wide)
    esc = (1 << (64 // (R + 1))) - 1
    assert ((e.read("head") - e.read("commit"))[wide] >= esc - 1).all() and not e.read("fault")[wide].any()
    tick(e, 0, everybody)
    rows = feed.settle("the wide commit catches up")
    assert has(rows, wide, LEADS | COMMITTED) and (rows["commit"] - rows["commit_from"] > 3 << 19).all()
    # followers: three blocks, then a Heartbeat that commits two of them
    lid = ids[(slots[fs].astype(np.int64) + 1) % R]
    for g, l in zip(fs, lid):
        e.submit(int(g), Command.AppendEntries(1, int(l), [(1, 0), (2, 1), (3, 2)]))
    e.step(500)
    drain_all(e)
    rows = feed.settle("followers appended")
    assert has(rows, fs, APPENDED, LEADS | COMMITTED) and (rows["head"] == 3).all()
    for g, l in zip(fs, lid):
        e.submit(int(g), Command.Heartbeat(1, 2, int(l)))
    e.step(600)
    drain_all(e)
    rows = feed.settle("followers advanced by Heartbeat")
    assert has(rows, fs, COMMITTED, LEADS | APPENDED) and (rows["commit"] == 2).all() and (rows["role"] == capi.ROLE_FOLLOWER).all()
    # a restart of followers with head > commit: the head goes down; some of them then stand for election before the feed
    # is read - a candidate's row
    back = fs[4:10].astype(np.uint32)
    assert (e.read("head")[back] > e.read("commit")[back]).all()
    e.submit_columns(np.full(len(back), capi.CMD_RESTART, np.uint8), back)
    e.step(5100)
    drain_all(e)
    cand = back[:3]
    e.submit_columns(np.full(len(cand), capi.CMD_TIMEOUT, np.uint8), cand)
    e.step(5150)
    drain_all(e)
    assert (e.read("role")[cand] == capi.ROLE_CANDIDATE).all()
    rows = feed.settle("restarted")
    assert has(rows, back, REWOUND, COMMITTED | APPENDED) and (rows["head"] == rows["commit"]).all() and (rows["head_from"] == 3).all()
    assert (rows["role"][np.isin(rows["group"], cand)] == capi.ROLE_CANDIDATE).all()
    # a recreate of followers and of leaders: genesis again
    again = np.concatenate([fs[10:14], gs[6:10]]).astype(np.uint32)
    again.sort()
    e.submit_columns(np.full(len(again), capi.CMD_RECREATE, np.uint8), again)
    e.step(5200)
    drain_all(e)
    rows = feed.settle("recreated")
    assert has(rows, again, REWOUND, COMMITTED | APPENDED | LEADS) and (rows["head"] == 0).all() and (rows["commit"] == 0).all()
    # a reference fault and an engine fault: an append the feed has not delivered yet, then the fault - the rows say FAULTED
    # with the columns as they froze, and nothing follows
    bad, eng = gs[10:13].astype(np.uint32), gs[13:16]
    tick(e, 1, everybody)
    e.submit_columns(np.full(len(bad), capi.CMD_APPEND_RESPONSE, np.uint8), bad, from_=np.full(len(bad), 77, np.uint32),
                     term=e.read("term")[bad].astype(np.uint64), id=np.ones(len(bad), np.uint64), flag=np.ones(len(bad), np.uint8))
    e.step(5300)
    drain_all(e)
    acks = np.full((R, G), capi.NO_ACK, np.uint64)
    acks[slots.astype(np.int64), at] = 0
    acks[slots[eng].astype(np.int64), eng] = capi.MAX_DENSE_APPENDS  # (too many appends: JG_FAULT_ENGINE_DENSE_APPENDS)
    e.step_dense_acks(acks)
    drain_all(e)
    fault = e.read("fault")
    assert ((fault[bad] > 0) & (fault[bad] < 128)).all() and (fault[eng] >= 128).all() and (fault[eng] != VAC).all()
    rows = feed.settle("faulted")
    assert has(rows, np.concatenate([bad, eng]), FAULTED | APPENDED, LEADS | VACANT | REWOUND)
    tick(e, 2, everybody)
    rows = feed.settle("the healthy leaders go on, the faulted slots' columns are frozen")
    assert not np.isin(rows["group"], np.concatenate([bad, eng])).any() and len(rows)
    # close: VACANT | REWOUND, view (0, 0); open: nothing (genesis only); load: the tree's commit and head
    shut = np.concatenate([gs[20:26], fs[20:26], bad[:1]])
    shut.sort()
    e.close_groups(shut)
    rows = feed.settle("closed")
    assert has(rows, shut, VACANT | REWOUND, COMMITTED | APPENDED | LEADS | FAULTED) and len(rows) == len(shut)
    assert (rows["commit"] == 0).all() and (rows["head"] == 0).all()
    e.open_groups(shut, 6000)
    assert len(feed.settle("opened: genesis only")) == 0
    trees = [([(0, 0)] + [(i, i - 1) for i in range(1, k + 11)], k + 9) for k in range(8)]
    e.load_chains(trees, now_ms=6100, g0=int(shut[0]))
    rows = feed.settle("loaded")
    assert len(rows) == 8 and rows["group"].tolist() == list(range(int(shut[0]), int(shut[0]) + 8))
    assert (rows["head"] == np.arange(8) + 9).all() and (rows["commit"] == np.arange(8) + 9).all()  # (Chain::new: head = commit)


def test_small_one_replica():
    G = 40
    e = BatchedRaft(G, 1, seed=2)
    feed = Feed(e)
    assert len(feed.settle("fresh")) == 0
    elect((e,), np.arange(G), 10)
    dense_tick((e,), 4, lambda k, head, slot: head)
    rows = feed.settle("a majority of one")
    assert has(rows, np.arange(G), LEADS | COMMITTED | APPENDED) and (rows["commit"] == 4).all() and (rows["head"] == 4).all()
    e.apply_all(Command.Recreate(), 100)
    drain_all(e)
    rows = feed.settle("recreated")
    assert has(rows, np.arange(G), REWOUND, LEADS | COMMITTED | APPENDED)


# ---- 3. values that differ only above bit 32, ids near 2^56 ---------------------------------------------------------------
def test_small_wide_values():
    G, R = 8, 3
    e = BatchedRaft(G, R, seed=1)
    feed = Feed(e)
    run = [(0, 0)] + [(i, i - 1) for i in range(1, 6)]
    hi, top = (1 << 32) + 5, 1 << 56
    e.load_chains([(run, 5)] * 4, now_ms=10)
    rows = feed.settle("commit 5, head 5")
    assert len(rows) == 4 and (rows["commit"] == 5).all() and (rows["head"] == 5).all()
    # the head alone moves, by 2^32 exactly: the low halves are equal
    for g in (0, 1):
        e.submit(g, Command.AppendEntries(1, 2, [(hi, 5)]))
    e.step(20)
    drain_all(e)
    assert e.read("head")[:2].tolist() == [hi, hi] and e.read("commit")[:2].tolist() == [5, 5]
    assert len(feed.poll("commits only: the head is not looked at", commits_only=True)) == 0
    rows = feed.settle("head 2^32 + 5")
    assert rows["group"].tolist() == [0, 1] and (rows["state"] == APPENDED).all() and (rows["head_from"] == 5).all()
    # ... then the commit alone, by 2^32 exactly
    for g in (0, 1):
        e.submit(g, Command.Heartbeat(1, hi, 2))
    e.step(30)
    drain_all(e)
    assert e.read("commit")[:2].tolist() == [hi, hi]
    rows = feed.settle("commit 2^32 + 5")
    assert rows["group"].tolist() == [0, 1] and (rows["state"] == COMMITTED).all() and (rows["commit_from"] == 5).all()
    # ... and both back down by 2^32 exactly: REWOUND
    e.load_chains([(run, 5)], now_ms=40)
    rows = feed.settle("back at 5")
    assert rows["group"].tolist() == [0] and (rows["state"] == REWOUND).all() and (rows["commit_from"] == hi).all()
    # ids near 2^56
    big = [(0, 0), (1, 0), (top - 1, 1), (top, top - 1)]
    e.load_chains([(big, top), (big, 1)], now_ms=50, g0=4)
    rows = feed.settle("ids near 2^56")
    assert rows["group"].tolist() == [4, 5] and rows["commit"].tolist() == [top, 1] and rows["head"].tolist() == [top, 1]
    e.submit(4, Command.AppendEntries(1, 2, [(top + 1, top)]))
    e.submit(4, Command.Heartbeat(1, top + 1, 2))
    e.step(2000)
    drain_all(e)
    rows = feed.settle("a block on top, committed")
    assert rows["group"].tolist() == [4] and rows["commit"].tolist() == [top + 1] and rows["state"].tolist() == [COMMITTED | APPENDED]


# ---- 4. the compaction: ranges and caps off the tile borders, delivery rules ------------------------------------------------
def loaded(G, R, seed):
    """an engine whose slots hold, at random, genesis only (nothing to report) or a short committed run; k: its length"""
    rng = np.random.default_rng(seed)
    k = np.where(rng.random(G) < 0.6, rng.integers(1, 6, G), 0)
    e = BatchedRaft(G, R, seed=seed)
    e.load_chains([([(0, 0)] + [(i, i - 1) for i in range(1, n + 1)], n if n else None) for n in k.tolist()],
                  now_ms=10)
    return e, k


@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_ranges_caps_and_peek(R):
    G = GC
    e, k = loaded(G, R, 20 + R)
    feed = Feed(e)
    assert (e.read("head") == k).all() and (e.read("commit") == k).all()
    pending = int((k > 0).sum())
    for g0, n in ((0, G), (1, G - 1), (3, 0), (G - 5, 5), (1000, 60)):
        for cap in (0, 1, 61, 256, 1024, 1030, None):
            for co in (False, True):
                feed.poll("peek", g0=g0, n=n, limit=cap, peek=True, commits_only=co)  # a peek advances nothing
    assert e.watch_commits(limit=0)[1] == pending
    rows = feed.poll("a range across the tile border is delivered, and only it", g0=1000, n=60)
    assert len(rows) == int((k[1000:1060] > 0).sum()) > 0
    pending -= len(rows)
    got = []
    for cap in (0, 1, 61, 256, 1024, 1030):  # a small cap loses nothing
        _, total, b0 = e.watch_commits(limit=0, backlog=True)  # the backlog with cap 0 ...
        rows, total1, b1 = e.watch_commits(limit=cap, peek=True, backlog=True)
        assert b0 == b1 and total == total1 == pending  # ... equals the backlog of the delivering call that follows
        rows = feed.poll(f"cap {cap}", limit=cap)
        assert len(rows) == min(cap, pending)
        pending -= len(rows)
        got.append(rows)
    assert pending == 0 and len(feed.settle("quiet")) == 0
    allrows = np.concatenate(got)
    assert (np.diff(allrows["group"].astype(np.int64)) > 0).all()  # ascending over the calls: nothing lost, nothing twice
    twin, _ = loaded(G, R, 20 + R)
    twin.watch_commits(1000, 60)
    same(allrows, twin.watch_commits()[0], "the union over the calls is one big call")
    # a delivered slot is silent until its view changes again
    gs = np.array([0, 5, 1023, 1024, 1025, 2047, 2048, G - 1], np.uint32)
    e.submit_columns(np.full(len(gs), capi.CMD_RECREATE, np.uint8), gs)
    e.step(100)
    drain_all(e)
    rows = feed.settle("recreated")
    assert rows["group"].tolist() == gs[k[gs] > 0].tolist() and (rows["state"] & REWOUND).all()


def test_small_commits_only():
    G, R = 96, 3
    e = BatchedRaft(G, R, seed=3, self_slots=(np.arange(G) % R).astype(np.uint8))
    feed = Feed(e)
    elect((e,), np.arange(G), 10)
    feed.settle("elected")
    half = np.arange(G) < G // 2
    # everybody appends; the acks of the first half arrive
    dense_tick((e,), 2, lambda k, head, slot: head)
    dense_tick((e,), 2, lambda k, head, slot: np.where(half, head, capi.NO_ACK).astype(np.uint64))
    assert len(feed.poll("peek", peek=True)) == G
    rows = feed.poll("commits only", commits_only=True)
    assert rows["group"].tolist() == np.nonzero(half)[0].tolist() and ((rows["state"] & (COMMITTED | APPENDED)) == (COMMITTED | APPENDED)).all()
    # both shadow words of the delivered slots advanced: they are silent now, with and without the flag
    rows = feed.poll("the appends of the other half")
    assert rows["group"].tolist() == np.nonzero(~half)[0].tolist() and ((rows["state"] & (COMMITTED | APPENDED)) == APPENDED).all()
    assert len(feed.settle("quiet")) == 0


# ---- 5. the feed IS the missing fsm_tx ----------------------------------------------------------------------------------------
def keys_of(fsm, G):
    """per partition the Apply keys and the Notify block ids of FSM rows, in order"""
    apply, notify = [[] for _ in range(G)], [[] for _ in range(G)]
    for r in expand_fsm_rows(fsm):
        g, a, b = int(r["group"]), int(r["a"]), int(r["b"])
        if r["kind"] == capi.FSM_APPLY_LEADER:
            apply[g] += range(a + 1, b + 1)
        elif r["kind"] == capi.FSM_APPLY_FOLLOWER:
            apply[g] += range(a, b)
        else:
            notify[g].append(a)
    return apply, notify


@pytest.mark.parametrize("every", [pytest.param(k, id=f"small-every-{k}") for k in (1, 3, 8)])
def test_the_feed_is_the_fsm_tx_of_dense_steps(every):
    G, R, T = 64, 3, 24
    rng = np.random.default_rng(every)
    slots = rng.integers(0, R, G).astype(np.uint8)
    a, _ = fresh(G, R, 9, slots)
    b, _ = fresh(G, R, 9, slots)
    lead = np.nonzero(rng.random(G) < 0.8)[0]
    for x in (a, b):
        elect((x,), lead, 10)
    ids = np.array(a.node_ids, np.uint32)
    feed = Feed(a)
    feed.settle("elected")
    apply_a, notify_a = [[] for _ in range(G)], [[] for _ in range(G)]
    apply_b, notify_b = [[] for _ in range(G)], [[] for _ in range(G)]
    at = np.arange(G)
    for t in range(T):
        head, term = a.read("head").astype(np.uint64), a.read("term").astype(np.uint64)
        acks = np.full((R, G), capi.NO_ACK, np.uint64)
        acks[slots.astype(np.int64), at] = 0
        acks[slots[lead].astype(np.int64), lead] = rng.integers(0, 4, len(lead))
        for k in range(1, R):  # a ragged ack stream: some members silent, some behind the head
            on = lead[rng.random(len(lead)) < 0.6]
            acks[(slots[on].astype(np.int64) + k) % R, on] = head[on] - np.minimum(head[on], rng.integers(0, 3, len(on)).astype(np.uint64))
        a.step_dense_acks(acks)
        drain_all(a)
        for g in lead.tolist():  # the same traffic as commands: the appends, then the acks by ascending slot
            for _ in range(int(acks[slots[g], g])):
                b.submit(g, Command.ClientRequest(0))
            for r in range(R):
                if r != slots[g] and acks[r, g] != capi.NO_ACK:
                    b.submit(g, Command.AppendResponse(int(ids[r]), int(term[g]), int(acks[r, g]), True))
        b.step(100 + t)
        ap, no = keys_of(b.drain_applies(), G)
        b.drain_messages(), b.drain_faults()
        for g in range(G):
            apply_b[g] += ap[g]
            notify_b[g] += no[g]
        if (t + 1) % every == 0 or t == T - 1:
            rows = feed.settle(f"tick {t}")
            assert not (rows["state"] & REWOUND).any()
            ap, _ = keys_of(commit_rows_as_fsm(rows), G)
            for r in rows:
                g = int(r["group"])
                apply_a[g] += ap[g]
                notify_a[g] += range(int(r["head_from"]) + 1, int(r["head"]) + 1)
    compare_snapshots(a, b, "twins")
    assert apply_a == apply_b and notify_a == notify_b
    assert sum(len(x) for x in apply_b) > G and sum(len(x) for x in notify_b) > G


# ---- 6. watching changes nothing -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_fuzz_and_watching_changes_nothing(R):
    G = 96
    rng = np.random.default_rng(11 + R)
    slots = rng.integers(0, R, G).astype(np.uint8)
    a, _ = fresh(G, R, 5, slots)
    b, _ = fresh(G, R, 5, slots)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    for x in (a, b):
        elect((x,), np.arange(0, G, 2), 10)
    feed = Feed(a)

    def look(what):
        feed.poll(what + " peek", g0=10, n=50, limit=3, peek=True)
        feed.poll(what + " commits", commits_only=True, limit=20)
        feed.settle(what)

    def others(what):  # the other two feeds deliver the same rows with and without commit watches in between
        for fn, args in (("watch_leaders", ()), ("watch_replicas", (2, 0))):
            x, y = getattr(a, fn)(*args), getattr(b, fn)(*args)
            assert x[1] == y[1] and x[0].tobytes() == y[0].tobytes(), (what, fn)

    now, kinds = 10, 0
    for s in range(16):
        batch = random_batch(rng, b, 3 * G, foreign_voters=True, budget=budget)
        now += int(rng.integers(0, 300))
        for e in (a, b):
            e.submit_columns(**batch)
            e.step(now)
        look(f"step {s}")
        if s % 3 == 0:
            others(f"step {s}")
        look(f"step {s} again")
        kinds |= int(np.bitwise_or.reduce(view_of(a, np.zeros((G, 2), np.uint64))["state"]))
        for fn in DRAINS:
            assert getattr(a, fn)().tobytes() == getattr(b, fn)().tobytes(), (s, fn)
        compare_snapshots(a, b, f"step {s}")
    for t in range(8):  # node steps, JG_NODE_ASYNC: the watch settles the step
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
        others(f"node {t}")
        compare_drains(a, b, f"node {t}")
        compare_snapshots(a, b, f"node {t}")
    assert kinds & LEADS and kinds & FAULTED and kinds & COMMITTED


# ---- 7. the control plane: moves into watched slots ----------------------------------------------------------------------------
def test_small_moves():
    G, R = 192, 3
    src = BatchedRaft(G, R, seed=2)
    dst = BatchedRaft(G, R, seed=2, start_vacant=True)
    fs, fd = Feed(src), Feed(dst)
    elect((src,), np.arange(96), 10)
    tick(src, 3, lambda k: src.read("head"))
    tick(src, 1, lambda k: src.read("head"))
    assert len(fs.settle("source")) == 96 and len(fd.settle("start vacant")) == 0
    move_groups(src, dst, 80, 30, close_source=True)
    rows = fd.settle("imported")
    assert rows["group"].tolist() == list(range(80, 96)) and has(rows, np.arange(80, 96), LEADS | COMMITTED | APPENDED, REWOUND)
    assert (rows["commit"] == 3).all() and (rows["head"] == 4).all()
    rows = fs.settle("moved away")
    assert rows["group"].tolist() == list(range(80, 96)) and (rows["state"] == (VACANT | REWOUND)).all()
    # ... and a move over slots the destination's feed has seen at other values
    tick(dst, 5, lambda k: dst.read("head"))
    fd.settle("the destination goes on")
    dst.close_groups(range(80, 96))
    move_groups(src, dst, 0, 16, dst_g0=80)
    rows = fd.settle("imported over seen slots")
    assert rows["group"].tolist() == list(range(80, 96)) and (rows["state"] & REWOUND).all() and (rows["head"] == 4).all()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_small_refusals():
    G, R = 200, 3
    e, twin = BatchedRaft(G, R, seed=4), BatchedRaft(G, R, seed=4)
    for x in (e, twin):
        elect((x,), np.arange(50), 10)
        tick(x, 2, lambda k: x.read("head"))
    api, h = e.api, e._h
    poison = np.frombuffer(b"\x5a" * (48 * G), capi.COMMIT_ROW_DTYPE).copy()
    rows, total, b = poison.copy(), C.c_size_t(12345), capi.CommitBacklog(*([0x5a] * 6))
    watch = lambda flags, g0, n, out, cap, tot: api.engine_watch_commits(h, flags, g0, n, out, cap, tot, C.byref(b))  # noqa: E731

    def untouched():
        return rows.tobytes() == poison.tobytes() and total.value == 12345 and all(getattr(b, k) == 0x5a for k in BACKLOG)

    T = C.byref(total)
    assert watch(0, 0, G, rows.ctypes.data, G, None) == capi.EINVAL            # a null total
    assert watch(0, 0, G, None, 5, T) == capi.EINVAL                           # a null out with cap > 0
    assert watch(4, 0, G, rows.ctypes.data, G, T) == capi.EINVAL               # an unknown flag
    assert watch(0x80000000, 0, G, rows.ctypes.data, G, T) == capi.EINVAL
    assert watch(0, G - 1, 2, rows.ctypes.data, G, T) == capi.EINVAL           # a range out of bounds
    assert watch(0, 1, 0xFFFFFFFF, rows.ctypes.data, G, T) == capi.EINVAL
    assert api.engine_watch_commits(None, 0, 0, G, rows.ctypes.data, G, T, C.byref(b)) == capi.EINVAL
    assert untouched()
    with pytest.raises(EngineError):
        e.watch_commits(g0=G, n=1)
    # kept node steps outstanding: refused with read_chains's code, and the kept steps are still viewable afterwards
    for x in (e, twin):
        x.step_node_begin(1000, async_=True, keep=True)
        x.step_node_begin(1100, async_=True, keep=True)
    r = capi.ChainRead()
    r.n, off = G, np.zeros(G + 1, np.uint64)
    r.off = off.ctypes.data
    code = api.engine_read_chains(h, C.byref(r), C.byref(C.c_uint64(0)))
    assert code == capi.EINVAL and watch(0, 0, G, rows.ctypes.data, G, T) == code and untouched()
    with pytest.raises(EngineError):
        e.watch_commits()
    outs = [[x.node_outbox(), x.node_outbox()] for x in (e, twin)]
    for k in range(2):
        for name, v in outs[0][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][k][name])), (k, name)
    compare_drains(e, twin, "kept")
    compare_snapshots(e, twin, "kept")
    # nothing was advanced by any of it: the feed still owes everything
    assert watch(capi.WATCH_PEEK, 0, G, None, 0, T) == capi.OK and total.value == 50 and b.changed == 50 and b.pending_appends == 100
    assert len(Feed(e).settle("after the refusals")) == 50
    assert api.engine_watch_commits(h, 0, 0, G, None, 0, T, None) == capi.OK and total.value == 0  # a null backlog is allowed


# ---- 9. shards ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [pytest.param(2, id="small-2-shards"), pytest.param(3, id="small-3-shards")])
def test_shards(D):
    G, R = 1003, 3
    s = BatchedRaft(G, R, seed=4, device_ids=[0] * D)
    one = BatchedRaft(G, R, seed=4)
    first, second = s.shard(0).G, s.shard(1).group_lo + s.shard(1).G

    def both(what, **kw):
        x, y = s.watch_commits(backlog=True, **kw), one.watch_commits(backlog=True, **kw)
        assert x[1] == y[1] and x[2] == y[2], (what, kw, x[1:], y[1:])
        same(x[0], y[0], what)
        return x

    assert both("fresh")[1] == 0
    for e in (s, one):
        elect((e,), np.arange(G), 10)
        dense_tick((e,), 3, lambda k, head, slot: head)
        dense_tick((e,), 1, lambda k, head, slot: np.where(np.arange(G) % 3 == 0, capi.NO_ACK, head).astype(np.uint64))
    assert both("count", limit=0)[1] == G
    both("a range across the shard border", g0=first - 5, n=11, peek=True)
    rows, total, _ = both("a cap that ends inside shard 0", limit=first // 2)
    assert total == G and rows["group"].tolist() == list(range(first // 2))
    rows, total, _ = both("peek", peek=True, limit=7)
    assert total == G - first // 2 and rows["group"][0] == first // 2  # the shards behind the cap kept their shadows
    rows, total, _ = both("a cap at the shard border", limit=first - first // 2)
    assert rows["group"][-1] == first - 1
    rows, total, _ = both("a cap inside shard 1", limit=(second - first) // 2)
    assert rows["group"][0] == first and rows["group"][-1] < second - 1
    rows, total, b = both("commits only", commits_only=True, limit=50)
    rows, total, b = both("the rest")
    assert rows["group"][-1] == G - 1 and b["changed"] == total
    assert both("quiet")[1] == 0
    for e in (s, one):
        dense_tick((e,), 2, lambda k, head, slot: head)
        e.close_groups(np.sort(np.random.default_rng(5).choice(G, 100, replace=False)))
    both("a cap of 1", limit=1)
    both("the last shard alone", g0=s.shard(D - 1).group_lo, n=G - s.shard(D - 1).group_lo, limit=3)
    rows, total, b = both("later deliveries")
    assert total > 100 and (np.diff(rows["group"].astype(np.int64)) > 0).all() and b["rewound"] > 0
    assert both("quiet")[1] == 0
    compare_snapshots(s, one, "shards")


# ---- 10. a node of a dense cluster, between rounds ----------------------------------------------------------------------------------
def test_small_cluster_nodes():
    from test_any_leader import spread_leaders
    G, R = 120, 3
    nodes = [BatchedRaft(G, R, seed=5 + r, self_slots=np.full(G, r, np.uint8), flags=capi.CFG_SEPARATE_COMMIT_KEY) for r in range(R)]
    spread_leaders(nodes, G, R)
    lib = DenseCluster(nodes, lead=None)
    lib.set_appends(per_group=(np.arange(G) % 4).astype(np.uint64))
    feeds = [Feed(e) for e in nodes]
    acc = np.zeros((R, G, 2), np.uint64)  # each node's (commit, head), accumulated from its feed alone
    now = 100
    for p in range(4):
        lib.rounds(now, 100, 8)
        now += 800
        for k, f in enumerate(feeds):
            rows = f.settle(f"poll {p} node {k}")
            g = rows["group"]
            assert (rows["commit_from"] == acc[k, g, 0]).all() and (rows["head_from"] == acc[k, g, 1]).all()
            assert not (rows["state"] & REWOUND).any()
            acc[k, g, 0], acc[k, g, 1] = rows["commit"], rows["head"]
            assert (acc[k, :, 0] == nodes[k].read("commit")).all() and (acc[k, :, 1] == nodes[k].read("head")).all()
            assert ((rows["state"] & LEADS) != 0).sum() > 0 and ((rows["state"] & LEADS) == 0).sum() > 0
    assert (acc[:, :, 0].max(axis=0)[np.arange(G) % 4 != 0] > 20).all()
    lib.close()


# ---- 11. full size (the device only) ----------------------------------------------------------------------------------------------------
def test_one_percent_moved_1m():
    from josefine_amd.traces import elect_all
    G, R = 1 << 20, 5
    rng = np.random.default_rng(6)
    e = BatchedRaft(G, R, seed=5, self_slots=(np.arange(G) % R).astype(np.uint8))
    elect_all(e, 10)
    drain_all(e)
    feed = Feed(e)
    dense_tick((e,), 3, lambda k, head, slot: head)
    dense_tick((e,), 0, lambda k, head, slot: head)
    assert len(feed.settle("everything moved")) == G
    moved = rng.random(G) < 0.01
    dense_tick((e,), np.where(moved, 2, 0), lambda k, head, slot: head)
    dense_tick((e,), 0, lambda k, head, slot: head)
    rows = feed.poll("one percent", limit=5000)
    assert len(rows) == 5000
    rows = feed.settle("the rest of it")
    assert len(rows) == int(moved.sum()) - 5000
