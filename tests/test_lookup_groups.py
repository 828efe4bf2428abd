"""Point queries (ABI v16): jg_engine_lookup_groups - the state of a list of slots in one call, in the order asked.  Every
field of a row named after a JG_FIELD_* is stated by code that existed before the call did: e.read(field) over the whole
engine, indexed with the list; `state` and `known_leader` by the leadership view of tests/test_leader_feed.py (view_of).
The engines are driven into every branch of the decode - leaders in lag space, with BEHIND and ABOVE escapes, with the run's
top as the lags' base, with the commit in the wide column; chains with an explicit id_gen; candidates, followers, queues,
faults, vacant slots - and the test asserts that each is among the slots compared.  Cases whose id contains "small" are
small enough for the emulated device (tests/test_lookup_groups_emulated.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

from josefine_amd import BatchedRaft, capi
from josefine_amd.engine import DeviceList, EngineError
from fuzz import random_batch
from parity import compare_drains, compare_snapshots
from test_leader_feed import view_of
from test_move_groups import drain_all
from test_replica_feed import elect
from test_vacant_groups import fresh

pytestmark = pytest.mark.gpu

VAC = capi.FAULT_VACANT
PIECE = 65536  # entries per staging piece (jg_api_lookup.h JG_LOOKUP_PIECE)
# the fields of a row that are a read(...) column, by the column's name
FIELDS = ("term", "head", "commit", "id_gen", "election_time", "heartbeat_time", "voted_for", "leader_id", "election_timeout",
          "queued_reqs", "role", "fault", "self_slot", "repl_state", "vote_seen", "vote_granted")
STATES = ("a leader wholly in lag space", "a leader with a BEHIND field", "a leader with an ABOVE field",
          "a leader whose base is run_hi", "a leader whose commit is in the wide column", "a non-FAST chain with explicit id_gen",
          "a candidate holding votes", "a follower that knows a leader and has voted", "a slot with queued requests",
          "a faulted slot", "a vacant slot")


def expected(e):
    """(rows[G], match[G, R]) of every slot of e from e.read(...) and the leadership view"""
    rows = np.zeros(e.G, capi.GROUP_STATE_DTYPE)
    rows["group"] = np.arange(e.G)
    for k in FIELDS:
        rows[k] = e.read(k)
    rows["has"] = e.read("has_voted") | (e.read("has_leader") << 1)
    v = view_of(e)
    rows["state"], rows["known_leader"] = v["state"], v["leader_id"]
    return rows, np.stack([e.read("match", r) for r in range(e.R)], axis=1)


def same(got, want, what=""):
    if got.tobytes() != want.tobytes():
        for k in got.dtype.names:
            bad = np.nonzero(got[k] != want[k])[0]
            assert not len(bad), (what, k, bad[:6], got[k][bad[:6]], want[k][bad[:6]])
    assert got.tobytes() == want.tobytes(), what


def tick(e, appends, ack):
    """one dense tick: every healthy leader appends appends[g] blocks; ack(k)[g]: what the member k behind the own slot
    acknowledges (NO_ACK: silent)"""
    G, R = e.G, e.R
    slot = e.read("self_slot").astype(np.int64)
    gs = np.nonzero((e.read("role") == capi.ROLE_LEADER) & (e.read("fault") == 0))[0]
    acks = np.full((R, G), capi.NO_ACK, np.uint64)
    acks[slot, np.arange(G)] = 0  # (the own slot carries the number of appends: none for a slot that does not lead)
    acks[slot[gs], gs] = np.broadcast_to(np.asarray(appends, np.uint64), (G,))[gs]
    for k in range(1, R):
        acks[(slot[gs] + k) % R, gs] = np.broadcast_to(np.asarray(ack(k), np.uint64), (G,))[gs]
    e.step_dense_acks(acks)
    drain_all(e)


def rows_to(e, gs, **cols):
    gs = np.asarray(gs, np.uint32)
    e.submit_columns(group=gs, **{k: np.broadcast_to(np.asarray(v), gs.shape).copy() for k, v in cols.items()})


class World:
    """an engine of 300 slots in every state the decode distinguishes, its expected rows, and which slots are in which"""


@functools.lru_cache(maxsize=None)
def world(R):
    G = 300
    rng = np.random.default_rng(40 + R)
    slots = rng.integers(0, R, G).astype(np.uint8)
    e, _ = fresh(G, R, 7 + R, slots)
    ids = np.array(e.node_ids, np.uint32)
    at = np.arange(G)
    sl = slots.astype(np.int64)
    esc = (1 << (64 // (R + 1))) - 1  # a lag field holds up to esc - 2 (R = 5: 1021, R = 3: 65533)
    no = np.uint64(capi.NO_ACK)
    # slots 0 .. 119 lead; everybody acknowledges a few appends
    elect((e,), at[:120], 10)
    for _ in range(2):
        tick(e, 3, lambda k: e.read("head"))
    # 20 .. 39: the member behind the own slot is down while the leaders append past the field limit (the others
    # acknowledge, so the commit follows); 40 .. 59: everybody is silent - the commit's lag leaves its field too
    down, silent = (at >= 20) & (at < 40), (at >= 40) & (at < 60)
    tick(e, np.where(down | silent, esc + 100, 2), lambda k: np.where(silent | (down & (k == 1)), no, e.read("head")))
    tick(e, 0, lambda k: np.where(silent | (down & (k == 1)), no, e.read("head")))
    # 60 .. 79: a forged ack above the head
    forged = (at >= 60) & (at < 80)
    tick(e, 0, lambda k: np.where(forged & (k == 1), e.read("head") + np.uint64(50), np.where(silent | (down & (k == 1)), no, e.read("head"))))
    # 80 .. 99: six appends nobody acknowledges, a restart (the head is back at the commit index, the run above it still
    # there), a second election, and an ack at the run's top
    again = at[80:100]
    tick(e, np.where((at >= 80) & (at < 100), 6, 0), lambda k: no)
    top = e.read("head")[again].astype(np.uint64)
    rows_to(e, again, kind=np.uint8(capi.CMD_RESTART))
    e.step(3000)
    drain_all(e)
    assert (e.read("head")[again] < top).all()
    elect((e,), again, 4000)
    rows_to(e, again, kind=np.uint8(capi.CMD_APPEND_RESPONSE), from_=ids[(sl[again] + 1) % R], term=e.read("term")[again].astype(np.uint64),
            id=top, flag=np.uint8(1))
    e.step(4100)
    drain_all(e)
    # 100 .. 104: an AppendResponse from a node the leader's progress does not know - a reference-domain fault
    rows_to(e, at[100:105], kind=np.uint8(capi.CMD_APPEND_RESPONSE), from_=np.uint32(77), term=e.read("term")[100:105].astype(np.uint64),
            id=np.uint64(1), flag=np.uint8(1))
    e.step(4200)
    drain_all(e)
    # 120 .. 129: candidates with their own vote and a refusal
    cand = at[120:130]
    rows_to(e, cand, kind=np.uint8(capi.CMD_TIMEOUT))
    e.step(4300)
    rows_to(e, cand, kind=np.uint8(capi.CMD_VOTE_RESPONSE), from_=ids[(sl[cand] + 1) % R], term=e.read("term")[cand].astype(np.uint64),
            flag=np.uint8(0))
    e.step(4300)
    drain_all(e)
    # 130 .. 299: the fuzzers' stream (candidates, followers that vote and learn leaders, queues, forks and gaps, faults)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    now = 4300
    for _ in range(14):
        b = random_batch(rng, e, 3 * G, foreign_voters=True, budget=budget)
        keep = b["group"] >= 130
        for k in ("kind", "group", "from_", "term", "id", "aux", "flag"):
            b[k] = b[k][keep]
        now += int(rng.integers(0, 300))
        e.submit_columns(**b)
        e.step(now)
        drain_all(e)
    # 280 .. 299 and a few leaders: closed
    e.close_groups(np.concatenate([at[280:300], at[110:114]]))
    w = World()
    w.e, w.R, w.G = e, R, G
    w.rows, w.match = expected(e)
    r = w.rows
    head, m = r["head"].astype(np.uint64), w.match.astype(np.uint64)
    lead = (r["role"] == capi.ROLE_LEADER) & (r["fault"] == 0)
    other = at[:, None] * 0 + np.arange(R)[None, :] != sl[:, None]  # [G, R]: the members but the own slot
    lag = np.where(m <= head[:, None], head[:, None] - np.minimum(m, head[:, None]), 0)
    restarted = np.isin(at, again)
    behind = (other & (lag >= esc - 1)).any(axis=1)
    above = (other & (m > head[:, None])).any(axis=1)
    unc = head - r["commit"]
    w.states = {
        "a leader wholly in lag space": lead & ~restarted & ~behind & ~above & (unc < esc - 1) & (head > 0),
        "a leader with a BEHIND field": lead & ~restarted & behind,
        "a leader with an ABOVE field": lead & ~restarted & above,
        # (the restarted leaders: genesis present, no window segment, not in RUN form - the acknowledged top is above the head)
        "a leader whose base is run_hi": lead & restarted & (m[at, (sl + 1) % R] == np.concatenate([np.zeros(80, np.uint64), top, np.zeros(G - 100, np.uint64)])),
        "a leader whose commit is in the wide column": lead & ~restarted & (unc >= esc - 1),
        "a non-FAST chain with explicit id_gen": (r["fault"] == 0) & (r["id_gen"] != head + 1),
        "a candidate holding votes": (r["role"] == capi.ROLE_CANDIDATE) & (r["fault"] == 0) & (r["vote_granted"] != 0),
        "a follower that knows a leader and has voted": (r["role"] == capi.ROLE_FOLLOWER) & (r["has"] == 3) & (r["fault"] == 0),
        "a slot with queued requests": r["queued_reqs"] > 0,
        "a faulted slot": (r["fault"] != 0) & (r["fault"] != VAC),
        "a vacant slot": r["fault"] == VAC,
    }
    return w


def raw(e, groups=None, g0=0, n=0, flags=0, out=None, match=None, device=None):
    """the C call itself: `groups` a host array, or `device` a device address"""
    s = capi.GroupSet()
    s.g0, s.n, s.flags = g0, n, flags
    if groups is not None:
        s.n, s.groups = len(groups), groups.ctypes.data
    if device is not None:
        s.groups, s.flags = device, flags | capi.GROUPS_DEVICE
    return e.api.engine_lookup_groups(e._h, C.byref(s), None if out is None else out.ctypes.data, None if match is None else match.ctypes.data)


def poison(n, R):
    return np.frombuffer(b"\x5a" * (80 * n), capi.GROUP_STATE_DTYPE).copy(), np.full((n, R), 0x5a5a5a5a5a5a5a5a, np.uint64)


# ---- 1. every decode branch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(5, id="small-5"), pytest.param(3, id="small-3")])
def test_every_decode_branch(R):
    w = world(R)
    missing = [k for k in STATES if not w.states[k].any()]
    assert not missing, missing  # a condition of the test: every state is among the slots compared
    rows, match = w.e.lookup(progress=True)  # the range form over the whole engine
    same(rows, w.rows, "range")
    assert match.tobytes() == w.match.tobytes()
    rng = np.random.default_rng(R)
    lst = rng.permutation(np.concatenate([np.arange(w.G)] * 3))[:800]
    for k in STATES:  # ... and a list that names at least one slot of every state
        assert w.states[k][lst].any(), k
    rows, match = w.e.lookup(lst, progress=True)
    same(rows, w.rows[lst], "list")
    assert match.tobytes() == w.match[lst].tobytes()
    same(w.e.lookup(lst), w.rows[lst], "list, no progress")


# ---- 2. list shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [pytest.param(n, id=f"small-{n}") for n in (1, 255, 256, 257, 1000)])
def test_list_shapes(n):
    w = world(5)
    rng = np.random.default_rng(n)
    lst = rng.integers(0, w.G, n) if n < 1000 else rng.permutation(np.concatenate([np.arange(w.G)] * 3 + [rng.integers(0, w.G, n - 3 * w.G)]))
    if n == 1000:
        assert len(lst) == n and np.bincount(lst, minlength=w.G).min() >= 3  # shuffled, and every slot repeats
    for kind in (list, np.int64, np.uint32):  # any integer sequence or array
        rows, match = w.e.lookup(kind(lst) if kind is list else lst.astype(kind), progress=True)
        same(rows, w.rows[lst], f"n = {n}")
        assert match.tobytes() == w.match[lst].tobytes()
    same(w.e.lookup(lst), w.rows[lst], f"n = {n}, no progress")
    # without the flag a match buffer is not touched
    out, m = poison(n, w.R)
    l32 = lst.astype(np.uint32)
    assert raw(w.e, l32, out=out, match=m) == capi.OK
    same(out, w.rows[lst])
    assert (m == 0x5a5a5a5a5a5a5a5a).all()


def test_small_range_form_and_empty():
    w = world(3)
    for g0, n in ((7, 257), (1, 299), (299, 1), (44, 0), (300, 0)):  # g0 > 0, n no multiple of 256
        rows, match = w.e.lookup(g0=g0, n=n, progress=True)
        same(rows, w.rows[g0:g0 + n], (g0, n))
        assert match.tobytes() == w.match[g0:g0 + n].tobytes()
    same(w.e.lookup(g0=200), w.rows[200:])
    # n = 0 is JG_OK, with nothing to write to
    assert len(w.e.lookup([])) == 0 and len(w.e.lookup(np.zeros(0, np.int64), progress=True)[1]) == 0
    assert raw(w.e, np.zeros(0, np.uint32)) == capi.OK and raw(w.e, g0=5, n=0) == capi.OK


def test_long_list_crosses_the_piece_boundary_twice():
    from node_step import elect_some
    G, R = 2000, 5
    rng = np.random.default_rng(8)
    e = BatchedRaft(G, R, seed=3, self_slots=rng.integers(0, R, G).astype(np.uint8))
    elect_some(e, rng.random(G) < 0.6, now_ms=10)
    drain_all(e)
    tick(e, rng.integers(0, 9, G), lambda k: e.read("head") - np.minimum(e.read("head"), rng.integers(0, 3, G).astype(np.uint64)))
    tick(e, rng.integers(0, 2000, G), lambda k: np.where(rng.random(G) < 0.3, np.uint64(capi.NO_ACK), e.read("head")))
    e.close_groups(np.sort(rng.choice(G, 100, replace=False)))
    want, wm = expected(e)
    lst = rng.integers(0, G, 2 * PIECE + 3)
    rows, match = e.lookup(lst, progress=True)
    same(rows, want[lst], "three pieces")
    assert match.tobytes() == wm[lst].tobytes()
    same(e.lookup(lst), want[lst], "three pieces, no progress")
    d = DeviceList(e, lst.astype(np.uint32))
    out, m = poison(len(lst), R)
    assert raw(e, n=len(lst), flags=capi.LOOKUP_PROGRESS, out=out, match=m, device=d.ptr) == capi.OK
    same(out, want[lst], "three pieces of a device list")
    assert m.tobytes() == wm[lst].tobytes()
    # an index out of range in the LAST position of a long device list: refused before the first piece is copied
    bad = lst.astype(np.uint32)
    bad[-1] = G
    d2 = DeviceList(e, bad)
    out, m = poison(len(lst), R)
    keep = out.tobytes(), m.tobytes()
    assert raw(e, n=len(lst), flags=capi.LOOKUP_PROGRESS, out=out, match=m, device=d2.ptr) == capi.EINVAL
    assert (out.tobytes(), m.tobytes()) == keep
    d.free(), d2.free()


# ---- 3. a device list ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(5, id="small-5"), pytest.param(3, id="small-3")])
def test_device_list(R):
    w = world(R)
    rng = np.random.default_rng(R + 20)
    for n in (1, 300, 700):
        lst = rng.integers(0, w.G, n)
        d = DeviceList(w.e, lst.astype(np.uint32))
        out, m = poison(n, R)
        assert raw(w.e, n=n, flags=capi.LOOKUP_PROGRESS, out=out, match=m, device=d.ptr) == capi.OK
        same(out, w.rows[lst], f"device list of {n}")
        assert m.tobytes() == w.match[lst].tobytes()
        same(out, w.e.lookup(lst), "the host list's rows")
        out, m = poison(n, R)
        assert raw(w.e, n=n, out=out, match=m, device=d.ptr) == capi.OK  # no progress: match stays as it was
        same(out, w.rows[lst])
        assert (m == 0x5a5a5a5a5a5a5a5a).all()
        d.free()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------
def test_small_refusals():
    w = world(3)
    e, G, R = w.e, w.G, w.R
    lst = np.arange(10, 60, dtype=np.uint32)
    n = len(lst)
    out, m = poison(n, R)
    keep = out.tobytes(), m.tobytes()
    P = capi.LOOKUP_PROGRESS
    bad_last, bad_first = lst.copy(), lst.copy()
    bad_last[-1], bad_first[0] = G, 0xFFFFFFFF
    dev_ok, dev_bad = DeviceList(e, lst), DeviceList(e, bad_last)
    cases = {
        "a null set": lambda: e.api.engine_lookup_groups(e._h, None, out.ctypes.data, m.ctypes.data),
        "a null out with n > 0": lambda: raw(e, lst, flags=P, out=None, match=m),
        "a null out with a range": lambda: raw(e, g0=0, n=5, out=None),
        "an unknown flag": lambda: raw(e, lst, flags=P | 4, out=out, match=m),
        "an unknown high flag": lambda: raw(e, lst, flags=1 << 31, out=out, match=m),
        "an index out of range, last": lambda: raw(e, bad_last, flags=P, out=out, match=m),
        "an index out of range, first": lambda: raw(e, bad_first, flags=P, out=out, match=m),
        "a range out of bounds": lambda: raw(e, g0=G - n + 1, n=n, flags=P, out=out, match=m),
        "a range that wraps": lambda: raw(e, g0=1, n=0xFFFFFFFF, flags=P, out=out, match=m),
        "progress without match": lambda: raw(e, lst, flags=P, out=out, match=None),
        "an index out of range in the last position of a device list": lambda: raw(e, n=n, flags=P, out=out, match=m, device=dev_bad.ptr),
        "the same without progress": lambda: raw(e, n=n, out=out, match=m, device=dev_bad.ptr),
    }
    for what, call in cases.items():
        assert call() == capi.EINVAL, what
        assert (out.tobytes(), m.tobytes()) == keep, what
    assert e.api.engine_lookup_groups(None, None, out.ctypes.data, None) == capi.EINVAL
    with pytest.raises(EngineError):
        e.lookup([0, G])
    with pytest.raises(EngineError):
        e.lookup([-1])
    with pytest.raises(EngineError):
        e.lookup(g0=G - 1, n=2)
    assert raw(e, n=n, flags=P, out=out, match=m, device=dev_ok.ptr) == capi.OK  # (the good device list goes through)
    same(out, w.rows[lst])
    dev_ok.free(), dev_bad.free()


def test_small_kept_and_async_node_steps():
    G, R = 200, 3
    e, twin = BatchedRaft(G, R, seed=4), BatchedRaft(G, R, seed=4)
    for x in (e, twin):
        elect((x,), np.arange(50), 10)
    # after a JG_NODE_ASYNC step the lookup is the settled state: read's
    rng = np.random.default_rng(3)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    for t in range(3):
        b = random_batch(rng, twin, G, foreign_voters=True, budget=budget)
        outs = []
        for x in (e, twin):
            x.submit_columns(**b)
            x.step_node_begin(1000 + 200 * t, async_=True)
            if x is e:
                got = e.lookup(progress=True)
            outs.append(x.node_outbox())
        for name, v in outs[0].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][name])), (t, name)
        want, wm = expected(e)
        same(got[0], want, f"async {t}")
        assert got[1].tobytes() == wm.tobytes()
        compare_drains(e, twin, f"async {t}")
        compare_snapshots(e, twin, f"async {t}")
    # kept node steps outstanding: refused with read_chains's code, and the kept steps are still viewable afterwards
    for x in (e, twin):
        x.step_node_begin(2000, async_=True, keep=True)
        x.step_node_begin(2100, async_=True, keep=True)
    r = capi.ChainRead()
    r.n, off = G, np.zeros(G + 1, np.uint64)
    r.off = off.ctypes.data
    code = e.api.engine_read_chains(e._h, C.byref(r), C.byref(C.c_uint64(0)))
    assert code == capi.EINVAL
    out, m = poison(G, R)
    keep = out.tobytes(), m.tobytes()
    assert raw(e, g0=0, n=G, flags=capi.LOOKUP_PROGRESS, out=out, match=m) == code
    assert raw(e, np.arange(5, dtype=np.uint32), out=out) == code
    assert (out.tobytes(), m.tobytes()) == keep
    with pytest.raises(EngineError):
        e.lookup()
    outs = [[x.node_outbox(), x.node_outbox()] for x in (e, twin)]
    for k in range(2):
        for name, v in outs[0][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][k][name])), (k, name)
    compare_drains(e, twin, "kept")
    compare_snapshots(e, twin, "kept")
    same(e.lookup(), expected(e)[0], "after the kept steps")


# ---- 5. it reads only ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("progress", [pytest.param(False, id="small-rows"), pytest.param(True, id="small-progress")])
def test_looking_up_changes_nothing(progress):
    G, R = 128, 3
    rng = np.random.default_rng(11)
    slots = rng.integers(0, R, G).astype(np.uint8)
    a, _ = fresh(G, R, 5, slots)
    b, _ = fresh(G, R, 5, slots)  # the twin nobody looks at
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    for x in (a, b):
        elect((x,), np.arange(0, G, 3), 10)

    def look(what):
        lst = rng.integers(0, G, 90)
        got = a.lookup(lst, progress=progress)
        want, wm = expected(a)
        same(got[0] if progress else got, want[lst], what)
        if progress:
            assert got[1].tobytes() == wm[lst].tobytes(), what
        a.lookup(g0=3, n=100, progress=progress)

    look("elected")
    now = 10
    for s in range(10):  # the general state machine
        batch = random_batch(rng, b, 3 * G, foreign_voters=True, budget=budget)
        now += int(rng.integers(0, 300))
        for e in (a, b):
            e.submit_columns(**batch)
            e.step(now)
        look(f"step {s}")
        compare_drains(a, b, f"step {s}")
    for t in range(4):  # dense ticks
        acks = np.full((R, G), capi.NO_ACK, np.uint64)
        some = rng.random(G) < 0.5
        acks[slots[some].astype(np.int64), np.nonzero(some)[0]] = 3
        acks[(slots[some].astype(np.int64) + 1) % R, np.nonzero(some)[0]] = b.read("head")[some]
        for e in (a, b):
            e.step_dense_acks(acks)
        look(f"dense {t}")
        compare_drains(a, b, f"dense {t}")
    for t in range(6):  # node steps, JG_NODE_ASYNC: the lookup settles the step
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
    compare_snapshots(a, b, "twin")
    assert a.read_chains()["off"].tobytes() == b.read_chains()["off"].tobytes()
    for fn, args in (("watch_leaders", ()), ("watch_replicas", (4, 1))):
        ra, rb = getattr(a, fn)(*args), getattr(b, fn)(*args)
        assert ra[1] == rb[1] and ra[0].tobytes() == rb[0].tobytes(), fn
    assert a.census() == b.census() and a.replication_census(2) == b.replication_census(2)
    compare_drains(a, b, "the end")


# ---- 6. a multi-device handle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [pytest.param(2, id="small-2-shards"), pytest.param(3, id="small-3-shards")])
def test_shards(D):
    from node_step import elect_some
    G, R = 1001, 3  # (ragged: the last shard owns fewer slots)
    rng = np.random.default_rng(D)
    s = BatchedRaft(G, R, seed=4, device_ids=[0] * D)
    one = BatchedRaft(G, R, seed=4)
    lead = rng.random(G) < 0.5
    shut = np.sort(rng.choice(G, 120, replace=False))
    for e in (s, one):
        elect_some(e, lead, now_ms=10)
        drain_all(e)
        tick(e, 4, lambda k: np.where((np.arange(G) % 3 == 0) & (k == 1), np.uint64(capi.NO_ACK), e.read("head")))
        tick(e, 70000 * (np.arange(G) % 5 == 0), lambda k: np.where(np.arange(G) % 2 == 0, np.uint64(capi.NO_ACK), e.read("head")))
        e.close_groups(shut)
    want, wm = expected(one)
    borders = np.array([s.shard(d).group_lo for d in range(1, D)])
    near = np.concatenate([borders - 1, borders, borders + 1, [0, G - 1]])
    lst = rng.permutation(np.concatenate([rng.integers(0, G, 1500), near, near]))  # repeats across the shard borders
    for progress in (True, False):
        a, b = s.lookup(lst, progress=progress), one.lookup(lst, progress=progress)
        ra, rb = (a[0], b[0]) if progress else (a, b)
        same(ra, rb, "the single engine's answer")
        same(ra, want[lst], "read's")
        if progress:
            assert a[1].tobytes() == b[1].tobytes() == wm[lst].tobytes()
    for g0, n in ((0, G), (int(borders[0]) - 3, 7), (1, G - 1), (G - 1, 1), (5, 0)):
        a, b = s.lookup(g0=g0, n=n, progress=True), one.lookup(g0=g0, n=n, progress=True)
        same(a[0], b[0], (g0, n))
        assert a[1].tobytes() == b[1].tobytes() == wm[g0:g0 + n].tobytes()
    # a device list on the parent is refused, whatever it points at; so are the other refusals, before any shard is asked
    out, m = poison(8, R)
    keep = out.tobytes(), m.tobytes()
    l8 = np.arange(8, dtype=np.uint32)
    assert raw(s, n=8, out=out, match=m, device=l8.ctypes.data) == capi.EINVAL
    l8[3] = G
    assert raw(s, l8, flags=capi.LOOKUP_PROGRESS, out=out, match=m) == capi.EINVAL
    assert (out.tobytes(), m.tobytes()) == keep
    compare_snapshots(s, one, "shards")
