"""Withdrawing waiters (ABI v24): jg_engine_await_cancel - a closed connection leaves the purgatory.  The statement is
tests/test_completion_feed.py's `Table` with one boolean per outstanding waiter, "marked", and rule 0 in front of its numpy
`view`: a marked waiter is CANCELLED and nothing else.  Every cancel is held to numpy (`marked` = the waiters NEWLY matching
`token & mask` among the keys), every watch to the view: the total, the rows byte for byte, all six stat words, what is
left.  Cases whose id contains "small" also run on the emulated device (tests/test_await_cancel_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, capi
from josefine_amd.engine import EngineError
from parity import compare_drains, compare_snapshots
from test_completion_feed import APPLIED, EXPIRED, FAULTED, LOST, TILE, VACANT, Table, committed_to
from test_lookup_groups import tick
from test_move_groups import drain_all
from test_replica_feed import dense_tick, elect
from test_vacant_groups import fresh

pytestmark = pytest.mark.gpu

CANCELLED = capi.DONE_CANCELLED
U = np.uint64
FULL = 2**64 - 1
HIGH = 0xFFFFFFFF00000000  # a connection id in the token's high half
W = 2 * TILE + 37          # three tiles of the mark pass, the last one ragged
KEYS_LDS = 2048            # jg_await.h JG_AWT_KEYS_LDS: up to here the keys are searched in LDS, beyond in device memory


class CancelTable(Table):
    """Table and, per outstanding waiter, whether a cancel has marked it"""

    def __init__(self, e, capacity):
        super().__init__(e, capacity)
        self.m = np.zeros(0, bool)

    def add(self, *a, **kw):
        super().add(*a, **kw)
        self.m = np.concatenate([self.m, np.zeros(len(self.w) - len(self.m), bool)])  # registered unmarked, whatever its token

    def plain(self, now_ms=0):
        return super().view(now_ms)

    def view(self, now_ms=0):
        v = super().view(now_ms)
        v["state"][self.m] = CANCELLED  # rule 0: that bit alone, whatever the slot looks like
        return v

    def watch(self, what="", now_ms=0, limit=None, peek=False):
        n0 = len(self.w)
        done = np.nonzero(self.view(now_ms)["state"] != 0)[0]
        rows = super().watch(what, now_ms, limit, peek)
        if len(self.w) != n0:  # the delivered waiters left: their marks with them
            keep = np.ones(n0, bool)
            keep[done[:len(rows)]] = False
            self.m = self.m[keep]
        assert len(self.m) == len(self.w)
        return rows

    def cancel(self, keys, mask=FULL, what=""):
        """one cancel held to numpy; `keys` as the caller passes them (any order, repeats)"""
        keys = np.asarray(keys, dtype=U)
        hit = np.isin(self.w["token"] & U(mask), keys)
        new = int((hit & ~self.m).sum())
        got = self.e.cancel_waiters(keys, mask)
        assert got == new, (what, got, new)
        self.m |= hit
        return got


def waiting_engine():
    """64 leaders at commit 40; block ids from 1000 wait"""
    return committed_to(64, 3, 3, 40)


# ---- 1. the search -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [pytest.param(k, id=f"small-{k}") for k in (1, 3, KEYS_LDS, KEYS_LDS + 1, 5000)])
def test_the_search(n_keys):
    e = waiting_engine()
    rng = np.random.default_rng(n_keys)
    tab = CancelTable(e, W)
    # tokens 100 apart, so that there is room for decoys between them - and the two ends of the key space, and the
    # neighbours of the first and the last key of call A
    base = (1000 + 100 * np.arange(W - 4)).astype(U)
    lo, hi = base[5], base[-7]
    tokens = np.concatenate([base, np.array([0, FULL, int(lo) - 1, int(hi) + 1], dtype=U)])
    tokens = tokens[rng.permutation(W)]
    tab.add(rng.integers(0, 64, W), 1000 + rng.integers(0, 50, W), tokens)

    def decoys(n, a, b):
        """n distinct values in (a, b) that are no token"""
        c = rng.choice(np.arange(a + 1, b), size=min(b - a - 1, 2 * n + 64), replace=False).astype(U)
        c = c[~np.isin(c, tokens)][:n]
        assert len(c) == n
        return c

    def passed(keys):
        """shuffled, and a quarter of them once more"""
        assert len(np.unique(keys)) == n_keys == len(keys)
        k = np.concatenate([keys, keys[rng.integers(0, len(keys), len(keys) // 4 + 2)]])
        return k[rng.permutation(len(k))]

    # A: the first and the last key are tokens; the tokens one below the first and one above the last are not marked
    between = base[(base > lo) & (base < hi)]
    if n_keys == 1:
        A = np.array([lo], dtype=U)
    else:
        real = rng.choice(between, size=min((n_keys - 2) // 3, 40), replace=False)
        A = np.concatenate([[lo, hi], real, decoys(n_keys - 2 - len(real), int(lo), int(hi))]).astype(U)
    n = tab.cancel(passed(A), what="A")
    assert n == (1 if n_keys == 1 else 2 + min((n_keys - 2) // 3, 40))
    assert tab.cancel(passed(A), what="A again") == 0  # a waiter that was marked already is not counted again
    by_token = dict(zip(tab.w["token"].tolist(), tab.m.tolist()))
    assert by_token[int(lo)] and not by_token[int(lo) - 1] and not by_token[int(hi) + 1] and (n_keys == 1 or by_token[int(hi)])
    # B: key sets that contain 0 and 2**64 - 1, and tokens equal to them
    if n_keys == 1:
        assert tab.cancel([0, 0], what="B: 0") == 1 and tab.cancel([FULL] * 3, what="B: ~0") == 1
    else:
        B = np.concatenate([np.array([0, FULL], dtype=U), decoys(n_keys - 2, 0, 200_000)])
        assert tab.cancel(passed(B), what="B") == 2
        assert tab.cancel(passed(B), what="B again") == 0
    by_token = dict(zip(tab.w["token"].tolist(), tab.m.tolist()))
    assert by_token[0] and by_token[FULL] and int(tab.m.sum()) == n + 2
    rows = tab.settle("the cancelled leave")
    assert len(rows) == n + 2 and (rows["state"] == CANCELLED).all() and not tab.m.any()
    assert {int(lo) - 1, int(hi) + 1} <= set(tab.w["token"].tolist())
    assert tab.cancel([0], 0, what="everything") == W - n - 2
    assert len(tab.settle("everything")) == W - n - 2
    tab.close()


# ---- 2. masks -------------------------------------------------------------------------------------------------------------------
def test_small_masks():
    e = waiting_engine()
    rng = np.random.default_rng(2)
    tab = CancelTable(e, W)
    conn = rng.integers(1, 8, W - 100)  # seven connections
    tokens = (conn.astype(U) << U(32)) | np.arange(W - 100, dtype=U)
    tab.add(rng.integers(0, 64, len(conn)), 1000, tokens)
    order = tab.w["token"].copy()
    # a key with a bit outside the mask is refused, and nothing is marked
    with pytest.raises(EngineError):
        e.cancel_waiters([2 << 32, (5 << 32) | 1], HIGH)
    tab.watch("after the refusal", peek=True)
    closed = np.array([2, 5], dtype=U) << U(32)
    n = tab.cancel(closed[::-1], HIGH, "two of seven connections")
    assert n == int(np.isin(conn, [2, 5]).sum()) and 100 < n < len(conn) - 100
    assert tab.cancel(closed, HIGH, "again") == 0
    # waiters registered after the cancel with matching tokens are not cancelled
    late = (U(2) << U(32)) | (np.arange(50, dtype=U) + U(1 << 20))
    tab.add(rng.integers(0, 64, 50), 1000, late)
    order = np.concatenate([order, late])
    # a peek removes nothing; a cap smaller than the number cancelled delivers the rest at the next watch
    assert len(tab.watch("peek", peek=True)) == n
    assert len(tab.watch("peek with a cap", limit=7, peek=True)) == 7
    first = tab.watch("a cap inside the cancelled", limit=n // 3)
    assert len(first) == n // 3 and int(tab.m.sum()) == n - n // 3  # the marks survived the compaction
    rest = tab.watch("the rest, with no cancel in between")
    assert len(rest) == n - n // 3 and not tab.m.any()
    got = np.concatenate([first, rest])
    assert (got["state"] == CANCELLED).all() and np.array_equal(got["token"], order[np.isin(order >> U(32), [2, 5]) & (order & U(1 << 20) == 0)])
    assert len(tab.settle("silent")) == 0
    # the survivors kept the registration order through the two compactions; mask 0 with key 0 marks everything left
    assert np.array_equal(tab.w["token"], order[np.isin(order, tab.w["token"])])
    left = len(tab.w)
    assert tab.cancel([0], 0, "everything left") == left and left == len(order) - n
    survivors = tab.w["token"].copy()
    rows = tab.settle("everything left")
    assert np.array_equal(rows["token"], survivors) and (rows["state"] == CANCELLED).all()
    e.open_waiters(0)  # nothing pins the table any more


# ---- 3. cancellation meets the feed ---------------------------------------------------------------------------------------------
def test_small_cancelled_whatever_the_slot_looks_like():
    G, R = 24, 3
    slots = (np.arange(G) % R).astype(np.uint8)
    e, _ = fresh(G, R, 4, slots)
    ids = np.array(e.node_ids, np.uint32)
    at = np.arange(G)
    elect((e,), at, 10)
    tick(e, 3, lambda k: e.read("head"))
    tick(e, 0, lambda k: e.read("head"))
    tick(e, 2, lambda k: capi.NO_ACK)  # uncommitted appends: ids 4 and 5
    assert (e.read("commit") == 3).all() and (e.read("head") == 5).all()
    term = e.read("term").astype(U)
    tab = CancelTable(e, 8 * G)
    kind = lambda k: (U(k) << U(32)) | at.astype(U)  # noqa: E731
    tab.add(at, 2, kind(1))                 # applied
    tab.add(at, 5, kind(2), 0, 50)          # past its deadline at 100
    tab.add(at, 4, kind(3), term)           # guarded: lost where the leader is deposed
    tab.add(at, 4, kind(4))                 # waits on a healthy leader: the waiter nothing else removes
    # [0, 8) deposed, [8, 12) closed, [12, 16) faulted (tests/test_completion_feed.py::test_small_lost_and_waiting)
    dep, shut, bad = at[:8], at[8:12], at[12:16].astype(np.uint32)
    e.submit_columns(np.full(len(dep), capi.CMD_RESTART, np.uint8), dep.astype(np.uint32))
    e.step(1000)
    drain_all(e)
    lid = ids[(slots[dep].astype(np.int64) + 1) % R]
    for g, l in zip(dep.tolist(), lid.tolist()):
        e.submit(g, Command.Heartbeat(int(term[0]) + 1, 3, l))
    e.step(1100)
    drain_all(e)
    e.close_groups(shut)
    e.submit_columns(np.full(len(bad), capi.CMD_APPEND_RESPONSE, np.uint8), bad, from_=np.full(len(bad), 77, np.uint32),
                     term=e.read("term")[bad].astype(U), id=np.ones(len(bad), U), flag=np.ones(len(bad), np.uint8))
    e.step(1400)
    drain_all(e)
    # every other waiter of every kind is withdrawn
    pick = tab.w["token"][(tab.w["token"] & U(1)) == 0]
    plain = tab.plain(100)
    gone = np.isin(tab.w["token"], pick)
    for s in (LOST | VACANT, LOST | FAULTED, LOST, APPLIED, EXPIRED, 0):  # a condition of the test: each is among the withdrawn
        assert (plain["state"][gone] == s).any(), s
    assert tab.cancel(pick, what="every other one") == len(pick) == 2 * G
    v = tab.view(100)
    assert (v["state"][gone] == CANCELLED).all() and set(np.unique(v["state"][~gone]).tolist()) == {LOST | VACANT, LOST | FAULTED, LOST, APPLIED, EXPIRED, 0}
    rows = tab.settle("cancelled and nothing else", now_ms=100)
    c = rows[rows["state"] == CANCELLED]
    assert len(c) == 2 * G and set(c["token"].tolist()) == set(pick.tolist())
    assert {capi.FAULT_VACANT} <= set(c["fault"].tolist()) and len(set(c["fault"].tolist())) >= 3  # the slot's fields as they are now
    assert len(tab.w) and np.isin(tab.w["token"] >> U(32), [3, 4]).all() and (tab.w["deadline_ms"] == 0).all()  # what waits for ever ...
    assert tab.cancel(np.array([4, 3], dtype=U) << U(32), HIGH, "the kinds") == len(tab.w)  # ... but for a cancel
    assert (tab.settle("the kinds")["state"] == CANCELLED).all() and not len(tab.w)
    tab.close()


# ---- 4. refusals and no side effects ----------------------------------------------------------------------------------------------
def test_small_refusals():
    G, R = 40, 3
    e, twin = (committed_to(G, R, 4, 3, capi.CFG_SEPARATE_COMMIT_KEY) for _ in range(2))  # (a leader's Tick then scans no commit key)
    api, h = e.api, e._h
    marked = C.c_size_t(12345)
    M = C.byref(marked)
    keys = np.array([11, 12], dtype=U)
    assert api.engine_await_cancel(h, keys.ctypes.data, 2, FULL, M) == capi.OK and marked.value == 0  # no table: nothing
    assert e.cancel_waiters([1, 2, 3]) == 0
    marked.value = 12345
    tab = CancelTable(e, 8)
    tab.add([1, 2, 3], [900, 900, 2], [11, 12, 13])
    many = np.arange(capi.AWAIT_CANCEL_MAX + 1, dtype=U)

    def refused(rc, what):
        assert rc == capi.EINVAL and marked.value == 12345, what
        tab.watch(what, peek=True)  # the next watch is unchanged: nothing was marked

    refused(api.engine_await_cancel(None, keys.ctypes.data, 2, FULL, M), "a null engine")
    refused(api.engine_await_cancel(h, keys.ctypes.data, 2, FULL, None), "a null marked")
    refused(api.engine_await_cancel(h, None, 2, FULL, M), "null keys")
    refused(api.engine_await_cancel(h, many.ctypes.data, len(many), FULL, M), "too many keys")
    refused(api.engine_await_cancel(h, keys.ctypes.data, 2, FULL ^ 1, M), "a key with a bit outside the mask")
    refused(api.engine_await_cancel(h, keys.ctypes.data, 2, 0, M), "a nonzero key under mask 0")
    assert api.engine_await_cancel(h, None, 0, FULL, M) == capi.OK and marked.value == 0  # no keys: nothing, and no launch
    assert api.engine_await_cancel(h, many.ctypes.data, capi.AWAIT_CANCEL_MAX, FULL, M) == capi.OK and marked.value == 3
    tab.m[:] = True
    assert tab.settle("the most keys")["state"].tolist() == [CANCELLED] * 3
    tab.add([1, 2, 3], [900, 900, 2], [11, 12, 13])
    marked.value = 12345
    # kept node steps outstanding: refused as the other synchronous calls are, and the kept steps are still viewable
    for x in (e, twin):
        x.step_node_begin(1000, async_=True, keep=True)
        x.step_node_begin(1100, async_=True, keep=True)
    assert api.engine_await_cancel(h, keys.ctypes.data, 2, FULL, M) == capi.EINVAL and marked.value == 12345
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        e.cancel_waiters([11])
    outs = [[x.node_outbox(), x.node_outbox()] for x in (e, twin)]
    for k in range(2):
        for name, v in outs[0][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][k][name])), (k, name)
    compare_drains(e, twin, "kept")
    compare_snapshots(e, twin, "kept")
    tab.watch("after the kept steps", peek=True)
    # a cancel and the watch behind it change nothing a step, a drain, a read or another feed can observe
    assert tab.cancel([12, 11, 12, 999], what="two of three") == 2
    rows = tab.watch("two cancelled, one applied")
    assert rows["state"].tolist() == [CANCELLED, CANCELLED, APPLIED]
    compare_snapshots(e, twin, "after a cancel and a watch")
    for x in (e, twin):
        dense_tick((x,), 1, lambda k, head, slot: head)
    compare_drains(e, twin, "a tick later")
    compare_snapshots(e, twin, "a tick later")
    tab.close()
    assert e.cancel_waiters([11]) == 0  # the table is gone


# ---- 5. multi-device ------------------------------------------------------------------------------------------------------------------
def test_small_shards():
    G, R, D = 100, 3, 3
    kw = dict(seed=4, self_slots=(np.arange(G) % R).astype(np.uint8))
    s = BatchedRaft(G, R, device_ids=[0] * D, **kw)
    one = BatchedRaft(G, R, **kw)
    los = [s.shard(d).group_lo for d in range(D)] + [G]
    rng = np.random.default_rng(8)
    n = 300
    gs = rng.integers(0, G, n)
    tokens = (rng.integers(1, 6, n).astype(U) << U(32)) | np.arange(n, dtype=U)
    for e in (s, one):
        elect((e,), np.arange(G), 10)
        dense_tick((e,), 4, lambda k, head, slot: head)
        e.open_waiters(n)  # (per shard on s)
        assert e.await_blocks(gs, 1000, tokens) == n
    owner = np.searchsorted(los, gs, side="right") - 1
    closed = np.isin(tokens >> U(32), [2, 4])
    assert all((closed & (owner == d)).any() for d in range(D))  # a condition of the test: every shard marks
    keys = np.array([4, 2, 4], dtype=U) << U(32)
    assert s.cancel_waiters(keys, HIGH) == one.cancel_waiters(keys, HIGH) == int(closed.sum())  # the sum over the shards
    assert s.cancel_waiters(keys, HIGH) == one.cancel_waiters(keys, HIGH) == 0
    exact = tokens[~closed][:40]
    assert s.cancel_waiters(exact) == one.cancel_waiters(exact) == 40
    x, y = s.watch_completions(0, stats=True), one.watch_completions(0, stats=True)
    assert x[1] == y[1] == int(closed.sum()) + 40 and x[2] == y[2] and x[2]["left"] == n - x[1]
    assert x[2]["applied"] == x[2]["lost"] == x[2]["expired"] == 0  # cancelled = done - applied - lost - expired
    assert sorted(x[0].tolist()) == sorted(y[0].tolist()) and (x[0]["state"] == CANCELLED).all()
    assert (x[0]["group"] == gs[(x[0]["token"] & U(0xFFFFFFFF)).astype(np.int64)]).all()  # the parent's index
    for d in range(D):  # per shard they arrive in registration order
        t = (x[0]["token"] & U(0xFFFFFFFF)).astype(np.int64)
        assert (np.diff(t[owner[t] == d]) > 0).all()
    assert s.cancel_waiters([0], 0) == one.cancel_waiters([0], 0) == n - x[1]
    x, y = s.watch_completions(0, stats=True), one.watch_completions(0, stats=True)
    assert x[1] == y[1] == n - int(closed.sum()) - 40 and x[2] == y[2] and x[2]["left"] == 0
    for e in (s, one):
        e.open_waiters(0)
    compare_snapshots(s, one, "shards")
