"""The completion feed (ABI v22): jg_engine_await_open / jg_engine_await_blocks / jg_engine_watch_completions - the
notifications of fsm::Driver (src/raft/fsm.rs:35, 56-84) as a table of waiters on the device.  A waiter's verdict is a
function of its slot's state as jg_read_state returns it, so the expected rows are stated in numpy over the engine's own
read(...) columns and a Python list of the outstanding waiters in registration order (`Table`): every watch is held to it -
the total, the rows (every field byte-equal, in order), the stats, what is left.  Cases whose id contains "small" are small
enough for the emulated device (tests/test_completion_feed_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, capi, expand_fsm_rows
from josefine_amd.engine import EngineError
from fuzz import random_batch
from parity import compare_drains, compare_snapshots
from test_lookup_groups import tick, world
from test_move_groups import drain_all
from test_replica_feed import dense_tick, elect
from test_vacant_groups import DRAINS, fresh
from wide_values import THI, elect_wide

pytestmark = pytest.mark.gpu

APPLIED, LOST, EXPIRED, VACANT, FAULTED = capi.DONE_APPLIED, capi.DONE_LOST, capi.DONE_EXPIRED, capi.DONE_VACANT, capi.DONE_FAULTED
TILE = 256  # waiters per tile of the passes (jg_await.h JG_AWT_TILE)
STATS = [name for name, _ in capi.AwaitStats._fields_]
U = np.uint64


def same(got, want, what=""):
    if got.tobytes() != want.tobytes():
        assert len(got) == len(want), (what, len(got), len(want))
        for k in got.dtype.names:
            bad = np.nonzero(got[k] != want[k])[0]
            assert not len(bad), (what, k, bad[:6], got[k][bad[:6]], want[k][bad[:6]])
    assert got.tobytes() == want.tobytes(), what


class Table:
    """the test's statement of one engine's feed: `w` is the outstanding waiters, in registration order"""

    def __init__(self, e, capacity):
        e.open_waiters(capacity)
        self.e, self.w = e, np.zeros(0, capi.AWAIT_ROW_DTYPE)

    def add(self, groups, block_ids, tokens, terms=0, deadlines_ms=0):
        groups = np.atleast_1d(np.asarray(groups))
        r = np.zeros(len(groups), capi.AWAIT_ROW_DTYPE)
        r["group"] = groups
        for k, v in (("block_id", block_ids), ("token", tokens), ("term", terms), ("deadline_ms", deadlines_ms)):
            r[k] = np.asarray(v, dtype=U)
        assert self.e.await_blocks(groups, block_ids, tokens, terms, deadlines_ms) == len(r)
        self.w = np.concatenate([self.w, r])

    def view(self, now_ms=0):
        """every outstanding waiter as the row a watch would deliver for it; state 0: it waits"""
        e, w = self.e, self.w
        g = w["group"].astype(np.int64)
        role, fault = e.read("role")[g], e.read("fault")[g]
        term, commit, head = e.read("term").astype(U)[g], e.read("commit").astype(U)[g], e.read("head").astype(U)[g]
        leads = role == capi.ROLE_LEADER
        guard, bid, dl = w["term"], w["block_id"], w["deadline_ms"]
        state = np.select([fault == capi.FAULT_VACANT, fault != 0, (guard != 0) & (~leads | (term != guard)),
                           np.where(leads, bid <= commit, bid < commit), (dl != 0) & (U(now_ms) >= dl)],
                          [LOST | VACANT, LOST | FAULTED, LOST, APPLIED, EXPIRED], 0)
        v = np.zeros(len(w), capi.DONE_ROW_DTYPE)
        v["group"], v["state"], v["role"], v["fault"], v["self_slot"] = w["group"], state, role, fault, e.read("self_slot")[g]
        v["token"], v["block_id"], v["term_now"], v["commit_now"], v["head_now"] = w["token"], bid, term, commit, head
        return v

    def watch(self, what="", now_ms=0, limit=None, peek=False):
        """one watch, held to numpy: the total, the rows, the stats, what is left; the delivered waiters leave unless
        peeking.  Returns the rows."""
        v = self.view(now_ms)
        done = v["state"] != 0
        want = v[done] if limit is None else v[done][:limit]
        rows, total, s = self.e.watch_completions(now_ms, limit, peek, stats=True)
        assert total == int(done.sum()), (what, total, int(done.sum()))
        same(rows, want, what)
        left = len(v) if peek else len(v) - len(want)
        exp = dict(waiting=int((~done).sum()), done=int(done.sum()), applied=int(((v["state"] & APPLIED) != 0).sum()),
                   lost=int(((v["state"] & LOST) != 0).sum()), expired=int(((v["state"] & EXPIRED) != 0).sum()), left=left)
        assert s == exp, (what, s, exp)
        if not peek and len(want):
            keep = np.ones(len(v), bool)
            keep[np.nonzero(done)[0][:len(want)]] = False
            self.w = self.w[keep]
        return rows

    def settle(self, what="", now_ms=0):
        """every done waiter is delivered; the feed is then silent"""
        rows = self.watch(what, now_ms)
        r2, total, s = self.e.watch_completions(now_ms, stats=True)
        assert total == 0 and len(r2) == 0 and s["left"] == len(self.w) and s["waiting"] == len(self.w), what
        return rows

    def close(self):
        self.settle("close", 0)
        rows, total = self.e.watch_completions(0, peek=True)
        assert total == 0
        if not len(self.w):
            self.e.open_waiters(0)


# ---- 1. every decode branch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(5, id="small-5"), pytest.param(3, id="small-3")])
def test_every_decode_branch(R):
    w = world(R)  # (test_lookup_groups: 300 slots in every state the decode of a leader's commit distinguishes)
    e = w.e
    commit, head, term = e.read("commit").astype(U), e.read("head").astype(U), e.read("term").astype(U)
    gs, ids, guards = [], [], []
    for g in range(w.G):
        for bid in (int(commit[g]) - 1, int(commit[g]), int(commit[g]) + 1, int(head[g]), int(head[g]) + 1):
            if bid <= 0:
                continue  # (block 0 is never applied: refused)
            for t in (0, int(term[g])):
                gs.append(g), ids.append(bid), guards.append(t)
    tab = Table(e, len(gs))
    far = 1 << 62  # (a deadline far away: the world is shared and stays as it is, so the waiters that wait leave by expiring at the end)
    tab.add(gs, ids, np.arange(len(gs)) + (7 << 40), guards, far)
    v = tab.view()
    among = np.zeros(w.G, bool)
    among[v["group"][v["state"] == APPLIED]] = True
    for k in ("a leader wholly in lag space", "a leader with a BEHIND field", "a leader with an ABOVE field", "a leader whose base is run_hi",
              "a leader whose commit is in the wide column", "a follower that knows a leader and has voted"):
        assert (w.states[k] & among).any(), k  # a condition of the test: the state is among the rows compared
    for bit in (VACANT, FAULTED):
        assert ((v["state"] & bit) != 0).any()
    assert (v["state"] == LOST).any() and (v["state"] == 0).any()
    tab.watch("the world, peeked", peek=True)
    tab.watch("the world, a few", limit=100)
    tab.settle("the world")
    assert len(tab.w) and (tab.view()["state"] == 0).all()
    rows = tab.settle("the end of time", now_ms=2**64 - 2)
    assert (rows["state"] == EXPIRED).all() and not len(tab.w)
    tab.close()


# ---- 2. compaction and cap -------------------------------------------------------------------------------------------------
def committed_to(G, R, seed, n, flags=0):
    """an engine of G leaders with commit = head = n"""
    e = BatchedRaft(G, R, seed=seed, self_slots=(np.arange(G) % R).astype(np.uint8), flags=flags)
    elect((e,), np.arange(G), 10)
    dense_tick((e,), n, lambda k, head, slot: head)
    dense_tick((e,), 0, lambda k, head, slot: head)
    assert (e.read("commit") == n).all()
    return e


@pytest.mark.parametrize("R", [pytest.param(3, id="small-3")])
def test_compaction_and_cap(R):
    G, W = 64, 2 * TILE + 37
    e = committed_to(G, R, 3, 40)
    rng = np.random.default_rng(5)
    tab = Table(e, W)
    token = 0
    # every round registers on the table as the round before compacted it (the buffers swapped), up to W waiters of which
    # about half - and the ones left waiting by the round before - are done
    for cap in (0, 1, 63, 64, 65, TILE, TILE + 1, "total - 1", "total", "total + 5"):
        commit = int(e.read("commit")[0])
        n = W - len(tab.w)
        tab.add(rng.integers(0, G, n), commit + rng.integers(-15, 16, n), np.arange(n) + token)
        token += n
        assert len(tab.w) == W
        with pytest.raises(EngineError):
            e.await_blocks([0], [1], [1])  # full
        total = e.watch_completions(limit=0)[1]
        assert TILE + 1 < total < W - 50
        if isinstance(cap, str):
            cap = eval(cap)  # noqa: S307
        tab.watch(f"peek {cap}", limit=cap, peek=True)  # a peek changes nothing
        before = tab.w["token"].copy()
        rows = tab.watch(f"cap {cap}", limit=cap)
        assert len(rows) == min(cap, total)
        assert np.array_equal(tab.w["token"], before[~np.isin(before, rows["token"])])  # the survivors' order is the registration order
        while e.watch_completions(limit=0)[1]:  # watches repeat until the feed is silent
            assert len(tab.watch(f"cap {cap} again", limit=max(cap, 60)))
        tab.settle("silent")
        assert np.array_equal(tab.w["token"], before[np.isin(before, tab.w["token"])]) and len(tab.w) > 100
        dense_tick((e,), 16, lambda k, head, slot: head)  # the commit passes the ones that wait
        dense_tick((e,), 0, lambda k, head, slot: head)
    rows = tab.settle("everything committed")
    assert not len(tab.w) and (rows["state"] == APPLIED).all()
    tab.close()


# ---- 3. the reference's Driver, differentially -------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(1, id="small-1"), pytest.param(3, id="small-3")])
def test_the_reference_driver(R):
    G, T = 64, 12
    rng = np.random.default_rng(R)
    slots = rng.integers(0, R, G).astype(np.uint8)
    e, _ = fresh(G, R, 9, slots)
    lead = np.arange(G)[rng.random(G) < 0.8]
    elect((e,), lead, 10)
    ids = np.array(e.node_ids, np.uint32)
    tab = Table(e, 4096)
    notifications = {}  # fsm.rs:35, keyed (group, block id)
    token, answered = 0, 0
    for t in range(T):
        head, term = e.read("head").astype(U), e.read("term").astype(U)
        for g in lead.tolist():
            for _ in range(int(rng.integers(0, 3))):
                e.submit(g, Command.ClientRequest(t))
            if R > 1 and rng.random() < 0.7:  # the appends of earlier steps are acknowledged by a majority
                for k in range(1, R // 2 + 1):
                    e.submit(g, Command.AppendResponse(int(ids[(slots[g] + k) % R]), int(term[g]), int(head[g]), True))
        e.step(100 + t)
        fsm = expand_fsm_rows(e.drain_applies())
        e.drain_messages(), e.drain_faults()
        responses, reg = set(), []
        for r in fsm:  # fsm.rs:56-84
            g, a, b = int(r["group"]), int(r["a"]), int(r["b"])
            if r["kind"] == capi.FSM_NOTIFY:
                token += 1
                notifications[(g, a)] = token
                reg.append((g, a, token))
            else:
                keys = range(a + 1, b + 1) if r["kind"] == capi.FSM_APPLY_LEADER else range(a, b)
                for k in keys:
                    if k and (g, k) in notifications:
                        responses.add(notifications.pop((g, k)))
        if reg:
            tab.add(*np.array(reg, dtype=np.int64).T)
        rows = tab.watch(f"step {t}")
        assert (rows["state"] == APPLIED).all()
        assert set(rows["token"].tolist()) == responses and len(rows) == len(responses), (t, sorted(rows["token"].tolist()), sorted(responses))
        answered += len(responses)
    assert not e.read("fault").any() and answered > G and token > answered - 1
    assert len(tab.w) == len(notifications)


# ---- 4. lost and waiting -------------------------------------------------------------------------------------------------------
def test_small_lost_and_waiting():
    G, R = 24, 3
    slots = (np.arange(G) % R).astype(np.uint8)
    e, _ = fresh(G, R, 4, slots)
    ids = np.array(e.node_ids, np.uint32)
    at = np.arange(G)
    elect((e,), at, 10)
    everybody = lambda k: e.read("head")  # noqa: E731
    tick(e, 3, everybody)
    tick(e, 0, everybody)
    tick(e, 2, lambda k: capi.NO_ACK)  # uncommitted appends: ids 4 and 5
    assert (e.read("commit") == 3).all() and (e.read("head") == 5).all()
    term = e.read("term").astype(U)
    tab = Table(e, 8 * G)
    tab.add(at, 4, at + 100, term)  # guarded
    tab.add(at, 4, at + 200, 0)     # the reference's rule
    tab.add(at, 4, at + 300, term + U(1))  # guarded by a leadership that is not the slot's
    rows = tab.settle("a wrong guard is lost at once; the others wait")
    assert sorted(rows["token"].tolist()) == (at + 300).tolist() and (rows["state"] == LOST).all()
    # the leaders of dep lose their leadership: the process restarts (a leader of the reference never steps down on a message:
    # leader.rs:248-266 ignores a Heartbeat), comes back a follower and learns of a leader at a higher term
    dep = at[:8]
    e.submit_columns(np.full(len(dep), capi.CMD_RESTART, np.uint8), dep.astype(np.uint32))
    e.step(1000)
    drain_all(e)
    lid = ids[(slots[dep].astype(np.int64) + 1) % R]
    nt = int(term[0]) + 1
    for g, l in zip(dep.tolist(), lid.tolist()):
        e.submit(g, Command.Heartbeat(nt, 3, l))
    e.step(1100)
    drain_all(e)
    assert (e.read("role")[dep] == capi.ROLE_FOLLOWER).all() and (e.read("term")[dep] == nt).all() and not e.read("fault").any()
    rows = tab.settle("deposed: the guarded waiter is lost, the other waits")
    assert sorted(rows["token"].tolist()) == (dep + 100).tolist() and (rows["state"] == LOST).all() and (rows["role"] == capi.ROLE_FOLLOWER).all()
    # the block commits on it as a follower: not done at commit == id, applied once commit > id (the half-open range)
    for g, l in zip(dep.tolist(), lid.tolist()):
        e.submit(g, Command.AppendEntries(nt, l, [(4, 3), (5, 4)]))
        e.submit(g, Command.Heartbeat(nt, 4, l))
    e.step(1200)
    drain_all(e)
    assert (e.read("commit")[dep] == 4).all() and not e.read("fault").any()
    assert len(tab.settle("a follower at commit == id: its Apply range is [from, commit)")) == 0
    for g, l in zip(dep.tolist(), lid.tolist()):
        e.submit(g, Command.Heartbeat(nt, 5, l))
    e.step(1300)
    drain_all(e)
    rows = tab.settle("a follower at commit > id")
    assert sorted(rows["token"].tolist()) == (dep + 200).tolist() and (rows["state"] == APPLIED).all()
    # a close: LOST | VACANT; a forged ack that faults the slot: LOST | FAULTED - guarded or not
    shut, bad = at[8:12], at[12:16].astype(np.uint32)
    e.close_groups(shut)
    e.submit_columns(np.full(len(bad), capi.CMD_APPEND_RESPONSE, np.uint8), bad, from_=np.full(len(bad), 77, np.uint32),
                     term=e.read("term")[bad].astype(U), id=np.ones(len(bad), U), flag=np.ones(len(bad), np.uint8))
    e.step(1400)
    drain_all(e)
    rows = tab.settle("closed and faulted")
    assert len(rows) == 16
    assert (rows["state"][np.isin(rows["group"], shut)] == (LOST | VACANT)).all() and (rows["state"][np.isin(rows["group"], bad)] == (LOST | FAULTED)).all()
    # the leaders that are left commit: at a leader commit == id is applied
    tick(e, 0, lambda k: np.where(at >= 16, 4, capi.NO_ACK).astype(U))
    assert (e.read("commit")[16:] == 4).all()
    rows = tab.settle("leaders at commit == id")
    assert len(rows) == 16 and (rows["state"] == APPLIED).all() and (rows["commit_now"] == 4).all() and not len(tab.w)
    tab.close()


# ---- 5. expiry -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("now", [pytest.param(5000, id="small-5000"), pytest.param(2**63 + 5, id="small-wide-clock")])
def test_expiry(now):
    G, R = 16, 3
    e = BatchedRaft(G, R, seed=6, self_slots=(np.arange(G) % R).astype(np.uint8))
    at = np.arange(G)
    elect_wide([e], THI, 10)  # a wide term (tests/wide_values.py)
    drain_all(e)
    assert (e.read("role") == capi.ROLE_LEADER).all() and (e.read("term") == THI).all()
    tick(e, 2, lambda k: e.read("head"))
    tick(e, 0, lambda k: e.read("head"))
    tick(e, 1, lambda k: capi.NO_ACK)
    assert (e.read("commit") == 2).all() and (e.read("head") == 3).all()
    tab = Table(e, 32 * G)
    token = 0
    for bid in (2, 3):  # applied / waiting
        for dl in (now - 1, now, now + 1, 0):
            for guard in (0, THI, THI ^ (1 << 32), THI ^ 1):
                tab.add(at, bid, at + token, guard, dl)
                token += G
    v = tab.view(now)
    for s in (APPLIED, EXPIRED, LOST, 0):
        assert (v["state"] == s).any()
    assert not ((v["state"] == EXPIRED) & (v["block_id"] == 2)).any()  # APPLIED beats EXPIRED
    tab.watch("before any deadline", now_ms=now - 2, peek=True)
    rows = tab.settle("at now", now_ms=now)
    assert set(np.unique(rows["state"]).tolist()) == {APPLIED, EXPIRED, LOST} and (rows["term_now"] == THI).all()
    assert len(tab.settle("again at now", now_ms=now)) == 0
    rows = tab.settle("a millisecond later", now_ms=now + 1)
    assert len(rows) == 2 * G and (rows["state"] == EXPIRED).all()
    assert len(tab.w) == 2 * G and (tab.w["deadline_ms"] == 0).all()  # without a deadline: never
    assert len(tab.settle("at the end of time", now_ms=2**64 - 2)) == 0
    tick(e, 0, lambda k: e.read("head"))
    assert len(tab.settle("committed", now_ms=now)) == 2 * G and not len(tab.w)
    tab.close()


# ---- 6. refusals and isolation ---------------------------------------------------------------------------------------------------
def test_small_refusals():
    G, R = 40, 3
    e, twin = (committed_to(G, R, 4, 3, capi.CFG_SEPARATE_COMMIT_KEY) for _ in range(2))  # (a leader's Tick then scans no commit key)
    api, h = e.api, e._h
    one = np.zeros(1, capi.AWAIT_ROW_DTYPE)
    one["block_id"], one["token"] = 2, 9
    reg = lambda r: api.engine_await_blocks(h, r.ctypes.data, len(r))  # noqa: E731
    assert reg(one) == capi.EINVAL  # no open table
    poison = np.frombuffer(b"\x5a" * (48 * 8), capi.DONE_ROW_DTYPE).copy()
    rows, total, s = poison.copy(), C.c_size_t(12345), capi.AwaitStats(*([0x5a] * 6))
    T = C.byref(total)
    watch = lambda flags, now, out, cap, tot: api.engine_watch_completions(h, flags, now, out, cap, tot, C.byref(s))  # noqa: E731

    def untouched():
        return rows.tobytes() == poison.tobytes() and total.value == 12345 and all(getattr(s, k) == 0x5a for k in STATS)

    assert api.engine_watch_completions(h, 0, 0, rows.ctypes.data, 8, T, None) == capi.OK and total.value == 0  # no table: nothing
    total.value = 12345
    tab = Table(e, 4)
    tab.add([1, 2], [2, 900], [11, 12])
    for field, value in (("group", G), ("group", 0xFFFFFFFF), ("flags", 1), ("reserved", 1), ("block_id", 0)):
        bad = np.concatenate([one, one])
        bad[field][1] = value
        assert reg(bad) == capi.EINVAL, field  # (the first row is fine: all or nothing)
    assert api.engine_await_blocks(h, None, 1) == capi.EINVAL and api.engine_await_blocks(None, one.ctypes.data, 1) == capi.EINVAL
    assert reg(np.concatenate([one] * 3)) == capi.ECAPACITY
    assert api.engine_await_blocks(h, None, 0) == capi.OK and reg(one[:0]) == capi.OK
    assert api.engine_await_open(h, 100) == capi.EINVAL and api.engine_await_open(h, 0) == capi.EINVAL  # waiters are outstanding
    assert api.engine_await_open(None, 4) == capi.EINVAL
    assert watch(0, 0, rows.ctypes.data, 8, None) == capi.EINVAL               # a null total
    assert watch(0, 0, None, 5, T) == capi.EINVAL                              # a null out with cap > 0
    assert watch(2, 0, rows.ctypes.data, 8, T) == capi.EINVAL                  # an unknown flag
    assert watch(0x80000000, 0, rows.ctypes.data, 8, T) == capi.EINVAL
    assert watch(0, 2**64 - 1, rows.ctypes.data, 8, T) == capi.EINVAL          # the clock's one refused value
    assert api.engine_watch_completions(None, 0, 0, rows.ctypes.data, 8, T, C.byref(s)) == capi.EINVAL
    assert untouched()
    # kept node steps outstanding: refused, and the kept steps are still viewable afterwards
    for x in (e, twin):
        x.step_node_begin(1000, async_=True, keep=True)
        x.step_node_begin(1100, async_=True, keep=True)
    assert watch(0, 0, rows.ctypes.data, 8, T) == capi.EINVAL and reg(one) == capi.EINVAL and untouched()
    assert api.engine_await_open(h, 0) == capi.EINVAL
    with pytest.raises(EngineError):
        e.watch_completions()
    outs = [[x.node_outbox(), x.node_outbox()] for x in (e, twin)]
    for k in range(2):
        for name, v in outs[0][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][k][name])), (k, name)
    compare_drains(e, twin, "kept")
    compare_snapshots(e, twin, "kept")
    # nothing was registered or removed by any of it
    rows2 = tab.settle("after the refusals")
    assert rows2["token"].tolist() == [11] and tab.w["token"].tolist() == [12]
    assert api.engine_watch_completions(h, 0, 0, None, 0, T, None) == capi.OK and total.value == 0  # null stats are allowed
    e.close_groups([2])
    assert tab.settle("closed")["state"].tolist() == [LOST | VACANT]
    tab.close()
    assert reg(one) == capi.EINVAL  # the table is gone


@pytest.mark.parametrize("R", [pytest.param(3, id="small-3")])
def test_fuzz_and_watching_changes_nothing(R):
    G = 96
    rng = np.random.default_rng(11 + R)
    slots = rng.integers(0, R, G).astype(np.uint8)
    a, _ = fresh(G, R, 5, slots)
    b, _ = fresh(G, R, 5, slots)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    for x in (a, b):
        elect((x,), np.arange(0, G, 2), 10)
    tab = Table(a, 4000)
    pick = np.random.default_rng(3)  # (the waiters' own stream: the batches are those of the commit feed's fuzz)
    token = [0]
    kinds = set()

    def look(what, now):
        n = 40
        g = pick.integers(0, G, n)
        head, term = a.read("head").astype(np.int64)[g], a.read("term").astype(U)[g]
        tab.add(g, np.maximum(head + pick.integers(-2, 3, n), 1), np.arange(n) + token[0], np.where(pick.random(n) < 0.5, term, 0),
                np.where(pick.random(n) < 0.3, np.maximum(now + pick.integers(-100, 400, n), 1), 0))
        token[0] += n
        tab.watch(what + " peek", now_ms=now, limit=3, peek=True)
        kinds.update(tab.watch(what, now_ms=now, limit=int(pick.integers(0, 60)))["state"].tolist())

    def others(what):  # the three other feeds deliver the same rows with and without completion watches in between
        for fn, args in (("watch_leaders", ()), ("watch_replicas", (2, 0)), ("watch_commits", ())):
            x, y = getattr(a, fn)(*args), getattr(b, fn)(*args)
            assert x[1] == y[1] and x[0].tobytes() == y[0].tobytes(), (what, fn)

    now = 10
    for s in range(16):
        batch = random_batch(rng, b, 3 * G, foreign_voters=True, budget=budget)
        now += int(rng.integers(0, 300))
        for e in (a, b):
            e.submit_columns(**batch)
            e.step(now)
        look(f"step {s}", now)
        if s % 3 == 0:
            others(f"step {s}")
        look(f"step {s} again", now)
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
                look(f"node {t}", now)
            outs.append(e.node_outbox())
        for name, x in outs[0].items():
            assert np.array_equal(np.asarray(x), np.asarray(outs[1][name])), (t, name)
        look(f"node {t} after", now)
        others(f"node {t}")
        compare_drains(a, b, f"node {t}")
        compare_snapshots(a, b, f"node {t}")
    assert {APPLIED, LOST, EXPIRED, LOST | FAULTED} <= kinds, kinds


# ---- 7. the dense path end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [pytest.param(120, id="small-120"), pytest.param(1000, id="1000")])
def test_dense_path_end_to_end(G):
    R, T = 5, 20
    rng = np.random.default_rng(7)
    e = BatchedRaft(G, R, seed=8, self_slots=(np.arange(G) % R).astype(np.uint8))
    elect((e,), np.arange(G), 10)
    e.watch_commits()
    tab = Table(e, 8 * G * 3)
    issued, answered_at, due = {}, {}, {}
    token = 0
    for t in range(T + 3):
        appends = rng.integers(0, 4, G) if t < T else 0
        lagging = rng.random(G) < 0.3  # some partitions' acks stay a tick behind
        dense_tick((e,), appends, lambda k, head, slot: np.where(lagging & (k <= 3) & (t < T), capi.NO_ACK, head).astype(U))
        rows, _ = e.watch_commits()
        app = rows[(rows["state"] & capi.CMT_APPENDED) != 0]
        n = (app["head"] - app["head_from"]).astype(np.int64)
        if n.sum():
            gs = np.repeat(app["group"], n)
            ids = np.concatenate([np.arange(int(r["head_from"]) + 1, int(r["head"]) + 1) for r in app])
            toks = np.arange(len(gs)) + token
            token += len(gs)
            tab.add(gs, ids, toks, np.repeat(app["term"], n))
            issued.update(zip(toks.tolist(), zip(gs.tolist(), ids.tolist())))
        commit = e.read("commit")
        for k, (g, bid) in issued.items():
            if k not in due and commit[g] >= bid:
                due[k] = t  # the first watch at which commit >= id
        for k in tab.watch(f"tick {t}")["token"].tolist():
            assert k not in answered_at
            answered_at[k] = t
    assert not len(tab.w) and len(issued) > G and set(answered_at) == set(issued)  # every token exactly once; the table is empty
    assert all(answered_at[k] == due[k] for k in issued)
    tab.close()


# ---- 8. multi-device ------------------------------------------------------------------------------------------------------------------
def test_small_shards():
    G, R, D = 100, 3, 3
    kw = dict(seed=4, self_slots=(np.arange(G) % R).astype(np.uint8))
    s = BatchedRaft(G, R, device_ids=[0] * D, **kw)
    one = BatchedRaft(G, R, **kw)
    los = [s.shard(d).group_lo for d in range(D)] + [G]
    rng = np.random.default_rng(8)
    n = 300
    gs, ids = rng.integers(0, G, n), rng.integers(1, 9, n)
    for e in (s, one):
        elect((e,), np.arange(G), 10)
        dense_tick((e,), 4, lambda k, head, slot: head)
        dense_tick((e,), 2, lambda k, head, slot: head)  # commit 4, head 6
        e.open_waiters(n)  # (per shard on s)
        assert e.await_blocks(gs, ids, np.arange(n), 0, np.where(ids > 6, 50, 0)) == n
    owner = np.searchsorted(los, gs, side="right") - 1
    per = [np.nonzero(owner == d)[0] for d in range(D)]  # the tokens of shard d, in registration order
    done = ids <= 4

    def both(what, now=0, **kw):
        x, y = s.watch_completions(now, stats=True, **kw), one.watch_completions(now, stats=True, **kw)
        assert x[1] == y[1], (what, x[1], y[1])
        return x, y

    (x, y) = both("count", limit=0)
    assert x[1] == int(done.sum()) and x[2] == y[2] and x[2]["left"] == n
    n0, n1 = int(done[per[0]].sum()), int(done[per[1]].sum())
    cap = n0 + n1 // 2  # runs out inside the second shard
    (x, y) = both("peek", limit=cap, peek=True)
    want = np.concatenate([per[0][done[per[0]]], per[1][done[per[1]]]])[:cap]
    assert x[0]["token"].tolist() == want.tolist()  # shard order, per shard in registration order
    (x, y) = both("a cap inside shard 1", limit=cap)
    assert x[0]["token"].tolist() == want.tolist() and x[2]["left"] == n - cap and x[2]["done"] == int(done.sum())
    assert (x[0]["group"] == gs[x[0]["token"]]).all()  # the parent's index
    got = [x[0]]
    (x2, y2) = both("the third shard kept its waiters", limit=0)
    assert x2[1] == int(done.sum()) - cap
    rest = s.watch_completions()
    got.append(rest[0])
    allrows = np.concatenate(got)
    ref = np.concatenate([y[0], one.watch_completions()[0]])
    assert sorted(allrows.tolist()) == sorted(ref.tolist()) and len(allrows) == int(done.sum())
    for d in range(D):  # per shard they arrive in registration order
        t = rest[0]["token"][owner[rest[0]["token"]] == d]
        assert (np.diff(t.astype(np.int64)) > 0).all()
    # expiry and a close across the shards
    for e in (s, one):
        e.close_groups(np.arange(30, 40))
    (x, y) = both("expired and closed", now=50)
    assert sorted(x[0].tolist()) == sorted(y[0].tolist()) and x[2] == y[2]
    assert set(np.unique(x[0]["state"]).tolist()) == {EXPIRED, LOST | VACANT}
    for e in (s, one):
        dense_tick((e,), 0, lambda k, head, slot: head)
    (x, y) = both("committed")
    assert sorted(x[0].tolist()) == sorted(y[0].tolist()) and x[2] == y[2] and x[2]["left"] == 0
    with pytest.raises(EngineError):
        s.await_blocks(np.full(n + 1, 5), 1, 0)  # one shard's table is full: nothing is registered anywhere
    assert s.watch_completions(limit=0, stats=True)[2]["left"] == 0
    compare_snapshots(s, one, "shards")
