"""Opening and closing partitions behind a kept node step (ABI v26): jg_step_node_hosted / jg_node_hosting_view - hosting
with two ticks in flight.

The hosted call defines no value of its own.  The reference is a TWIN, as in tests/test_node_lookup.py: a second device
engine of the same seed and config, fed the same rows and stepped synchronously, which after its step runs
close_groups(close) and then open_groups(open, now).  Kept step t - begun with the same two sets while step t - 1 was still
outstanding - hands out the twin's outbox and drains (the step itself sees the engine without the hosting pass), counts in
node_hosting() what the twin's calls wrote, and leaves the engine the twin's: every readable column every few ticks, the
export records byte for byte and the vacant / hosted lists at the end.  The cases with "small" in their ids also run on the
emulated device (tests/test_node_hosting_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import capi
from josefine_amd.engine import EngineError
from node_step import compare_outboxes, node_traffic
from parity import compare_snapshots
from test_lookup_groups import same
from test_node_await import answer_equal, waiters
from test_node_lookup import lookup_equal
from test_node_poll import DRAINS, EVERYTHING, steady, strip, twin_pair
from test_node_step import _same_rows
from test_poll import equal

pytestmark = pytest.mark.gpu

G = 1024 + 256 + 37
LENGTHS = (0, 1, 63, 64, 65, 257)  # around a wave, and more than one workgroup with a partial last one
KEPT = dict(async_=True, keep=True)
FLAGS = capi.NODE_LEADER_HALF | capi.NODE_FOLLOWER_HALF | capi.NODE_TICK | capi.NODE_ASYNC | capi.NODE_KEEP
NOTHING = dict(closed=0, opened=0, close_refused=False, open_refused=False)


def suffix(state_is, Gn, most=201):
    """the range that ends at G over the longest run of slots in the wanted state (at most `most` of them; may be empty)"""
    m = 0
    while m < min(most, Gn) and state_is[Gn - 1 - m]:
        m += 1
    return range(Gn - m, Gn)


def shape(case, t, rng, twin):
    """the hosting request of tick t from the twin's lists after its step: the list lengths and the range form that ends at
    G, cycling; the close and the open of a tick take different lengths"""
    hosted, vacant = twin.hosted_groups(), twin.vacant_groups()
    is_hosted = np.zeros(twin.G, bool)
    is_hosted[hosted] = True

    def pick(pool, k, state):
        if k < len(LENGTHS):
            return rng.choice(pool, min(LENGTHS[k], len(pool)), replace=False)
        return suffix(is_hosted == state, twin.G)

    req = {}
    if case in ("close", "both", "own", "everything"):
        req["close"] = pick(hosted, t % 7, True)
    if case in ("open", "both", "own", "everything"):
        pool = vacant
        if "close" in req and not isinstance(req["close"], range) and t % 2:  # some of what this very step closes is reopened
            pool = np.concatenate([vacant, np.asarray(req["close"], vacant.dtype)[:5]])
        k = (t + 3) % 7
        if k == 6 and "close" in req and isinstance(req["close"], range):
            k = 2
        req["open"] = pick(pool, k, False)
        if case == "own" and not isinstance(req["open"], range):  # own slots, the engine's uniform one and every other
            req["self_slots"] = rng.integers(0, twin.R, len(req["open"]))
    return req


def twin_hosting(twin, req, now):
    """the two synchronous calls on the twin; what node_hosting() must report of them"""
    res = dict(NOTHING)
    if req.get("close") is not None:
        try:
            twin.close_groups(req["close"])
            res["closed"] = len(req["close"])
        except EngineError:
            res["close_refused"] = True
    if req.get("open") is not None:
        try:
            twin.open_groups(req["open"], now, self_slots=req.get("self_slots"))
            res["opened"] = len(req["open"])
        except EngineError:
            res["open_refused"] = True
    return res


def same_engine(dev, twin, what):
    compare_snapshots(dev, twin, what)
    assert dev.export_groups().records.tobytes() == twin.export_groups().records.tobytes(), what
    assert np.array_equal(dev.vacant_groups(), twin.vacant_groups()) and np.array_equal(dev.hosted_groups(), twin.hosted_groups()), what


# (case, R, ticks, seed): the cases with "small" in their ids are R in {3, 5} and 6 ticks
CASES = [pytest.param("both", 3, 6, id="small-both-3"), pytest.param("own", 5, 6, id="small-own-5"),
         pytest.param("close", 3, 24, id="close-3"), pytest.param("open", 5, 24, id="open-5"), pytest.param("both", 8, 24, id="both-8"),
         pytest.param("own", 3, 24, id="own-3"), pytest.param("own", 8, 24, id="own-8"),
         pytest.param("everything", 3, 24, id="with-poll-completions-and-lookup-3")]


@pytest.mark.parametrize("case,R,T", CASES)
def test_hosted_steps_equal_the_twins_calls(case, R, T):
    """T ticks of node_traffic, two steps in flight, every step hosted: per tick the viewed outbox and the drains are the
    twin's, node_hosting() counts what the twin's close_groups and open_groups wrote after its synchronous step of that
    tick, and every few ticks and at the end the engine is the twin's.  Ticks whose rows took the general path come back
    "redone", the others do not, and both kinds write slots.  One case carries a poll, a completion request and a lookup on
    the same steps: all three see the engine without the step's own hosting pass, the next step's leader feed reports the
    change and its watch delivers the waiters of closed slots as JG_DONE_VACANT."""
    dev, twin, rng = twin_pair(G, R, seed=61 + R)
    pick = np.random.default_rng(13)  # (the sets' and the waiters' own stream)
    full = case == "everything"
    if case != "close":  # something to open from the first tick on
        gone = pick.choice(G, G // 2 if case == "open" else G // 4, replace=False)
        for e in (dev, twin):
            e.close_groups(gone)
    if full:
        for e in (dev, twin):
            e.open_waiters(900)
    want = []
    kinds = {True: [0, 0], False: [0, 0]}  # redone or not: ticks, slots written
    token = vacant_done = feed_vacant = 0

    def finish(t):
        nonlocal vacant_done, feed_vacant
        b, drains, res, look, looked, polled, answer = want[t]
        compare_outboxes(dev.node_outbox(), b, f"tick {t}")
        for fn in DRAINS:
            _same_rows(getattr(dev, fn)(), drains[fn], f"tick {t}: {fn}")
        got = dev.node_hosting()
        redone = got.pop("redone")
        assert got == res, (t, got, res)
        assert redone == (b["rows_general"] > 0), (t, redone, b["rows_general"])
        kinds[redone][0] += 1
        kinds[redone][1] += got["closed"] + got["opened"]
        if full:
            r2, p = strip(dev.node_poll())
            equal(p, polled, f"tick {t}: the poll")
            done = dev.node_completions()
            answer_equal(done["answer"], answer, f"tick {t}: the completions")
            lookup_equal(dev.node_lookup(), looked, look["progress"], f"tick {t}: the lookup")
            assert r2 == done["redone"] == redone
            vacant_done += int(((done["answer"][0]["state"] & capi.DONE_VACANT) != 0).sum())
            feed_vacant += int((p["leaders"][0]["fault"] == 255).sum())
        else:
            assert dev.node_poll() == {"redone": False} and dev.node_lookup() == {"redone": False}

    for t in range(T):
        now = 100 * (t + 1)
        cols = node_traffic(rng, twin, token0=1000 * t, p_noise=0.03 if t % 3 else 0.0, p_reorder=0.08 if t % 3 else 0.0)
        if t % 3 == 0:  # every third tick is all steady state: its hosting pass is the one queued behind the step, not redone
            cols = steady(cols, twin)
        poll = dict(EVERYTHING) if full else None
        request = look = None
        if full:
            new = waiters(pick, twin, 20, now, token, far=0.5)
            token += 20
            request = dict(new, now_ms=now, stats=True)
            look = dict(groups=pick.integers(0, G, 90), progress=bool(t % 2))
        twin.submit_columns(**cols)
        b = twin.step_node(now)
        drains = {fn: getattr(twin, fn)() for fn in DRAINS}
        polled = answer = looked = None
        if full:  # (all three on the engine as the step leaves it: the hosting calls come behind them)
            polled = twin.poll(**poll)
            assert twin.await_blocks(**new) == 20
            answer = twin.watch_completions(now, stats=True)
            looked = twin.lookup(**look)
        req = shape(case, t, pick, twin)
        res = twin_hosting(twin, req, now)
        assert not res["close_refused"] and not res["open_refused"], (t, res)
        want.append((b, drains, res, look, looked, polled, answer))
        dev.submit_columns(**cols)  # (the rows of tick t + 1 address what tick t opened: submitted before t is viewed)
        dev.step_node_begin(now, poll=poll, completions=request, lookup=look, hosting=req, **KEPT)
        if t % 5 == 4:  # a read between begin and view settles the newest step: the hosting pass is behind it
            compare_snapshots(dev, twin, f"tick {t}, read while it is outstanding")
        if t:
            finish(t - 1)
    finish(T - 1)
    same_engine(dev, twin, "after the last tick")
    for redone in (True, False):
        assert kinds[redone][0] >= 2 and kinds[redone][1] >= 1, kinds
    if full:
        assert vacant_done >= 1 and feed_vacant >= 1, (vacant_done, feed_vacant)
        equal(dev.poll(**EVERYTHING), twin.poll(**EVERYTHING), "one poll afterwards")


def pair(Gn=300, R=3, seed=5, vacant=()):
    dev, twin, rng = twin_pair(Gn, R, seed=seed)
    if len(vacant):
        for e in (dev, twin):
            e.close_groups(vacant)
    return dev, twin, rng


def rows_for(groups, kind=capi.CMD_TIMEOUT):
    return dict(kind=np.full(len(groups), kind, np.uint8), group=np.asarray(groups, np.uint32))


def twin_step(twin, now):
    return twin.step_node(now), {fn: getattr(twin, fn)() for fn in DRAINS}


def same_step(dev, got, want, what):
    compare_outboxes(got, want[0], what)
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), want[1][fn], f"{what}: {fn}")


def test_small_rows_of_the_step_and_of_the_next_one():
    """a slot closed by the step that carries general-path rows for it (applied first: it campaigns, then it is gone); rows
    for a vacant slot in the step that opens it (ignored); rows of tick t + 1 for a slot tick t opens, submitted before t
    is viewed (they meet the opened slot: it campaigns)"""
    V = np.arange(40, 60)
    dev, twin, rng = pair(vacant=V)
    A = np.array([3, 4, 5, 64, 255, 299])
    # step 1: Timeout rows for A (the general path) and for V[:6] (vacant: ignored), A closed and V[:6] opened behind it
    cols = rows_for(np.concatenate([A, V[:6]]))
    twin.submit_columns(**cols), dev.submit_columns(**cols)
    first = twin_step(twin, 100)
    assert first[0]["rows_general"] > 0 and set(first[1]["drain_messages"]["group"]) & set(A)  # (the closed slots' vote requests)
    assert not set(first[1]["drain_messages"]["group"]) & set(V)  # (a vacant slot ignores its rows)
    twin.close_groups(A), twin.open_groups(V[:6], 100)
    dev.step_node_begin(100, hosting=dict(close=A, open=V[:6]), **KEPT)
    # step 2, begun before step 1 is viewed: Timeout rows for the slots step 1 opened, and for the ones it closed
    cols = rows_for(np.concatenate([V[:6], A]))
    twin.submit_columns(**cols), dev.submit_columns(**cols)
    second = twin_step(twin, 200)
    said = set(second[1]["drain_messages"]["group"])  # (the opened slots campaign; the closed ones say nothing)
    assert set(V[:6]) <= said and not said & set(A), said
    dev.step_node_begin(200, **KEPT)
    same_step(dev, dev.node_outbox(), first, "the step that closes and opens")
    assert dev.node_hosting() == dict(NOTHING, redone=True, closed=len(A), opened=6)
    same_step(dev, dev.node_outbox(), second, "the step after")
    assert dev.node_hosting() == {"redone": False}
    same_engine(dev, twin, "afterwards")


def test_small_close_and_reopen_in_one_step():
    """one slot in both sets of a step: the open's check sees the close's writes; the draw count is carried (the export
    records are the twin's) and the timeout is a new draw"""
    dev, twin, rng = pair(seed=9)
    both = np.array([0, 7, 63, 64, 200, 299])
    before = dev.read("election_timeout")[both]
    records = dev.export_groups().records[both].copy()
    for now, rows in ((100, False), (200, True)):  # behind a step without rows, and behind one with general-path rows
        if rows:
            cols = rows_for([10, 11])
            twin.submit_columns(**cols), dev.submit_columns(**cols)
        want = twin_step(twin, now)
        assert (want[0]["rows_general"] > 0) == rows
        twin.close_groups(both), twin.open_groups(both, now)
        dev.step_node_begin(now, hosting=dict(close=both, open=both), **KEPT)
        same_step(dev, dev.node_outbox(), want, f"now={now}")
        assert dev.node_hosting() == dict(NOTHING, redone=rows, closed=len(both), opened=len(both))
        same_engine(dev, twin, f"now={now}")
        after = dev.read("election_timeout")[both]
        assert (after != before).sum() >= len(both) - 1, (before, after)  # (a draw of ~800 values may repeat once)
        assert (dev.read("fault")[both] == 0).all()
        now_records = dev.export_groups().records[both]
        assert all(a.tobytes() != b.tobytes() for a, b in zip(now_records, records))
        before, records = after, now_records.copy()


def test_small_refused_sets():
    """a set the synchronous call refuses for a slot's state writes nothing and says so with the view; the other set is
    applied; the engine is the twin's"""
    V = np.arange(100, 130)
    dev, twin, rng = pair(seed=7, vacant=V)
    for t, (req, res) in enumerate((
            (dict(close=[1, 2, 100, 200], open=V[5:9]), dict(NOTHING, close_refused=True, opened=4)),     # 100 is vacant
            (dict(close=[1, 2, 200], open=[99, 110, 111]), dict(NOTHING, closed=3, open_refused=True)),   # 99 is hosted
            (dict(close=range(90, 101), open=range(100, 106)), dict(NOTHING, close_refused=True, open_refused=True)),
            (dict(close=[50], open=[50, 51]), dict(NOTHING, closed=1, open_refused=True)),                # 51 is hosted
            (dict(open=[120], self_slots=[2]), dict(NOTHING, opened=1)))):
        now = 100 * (t + 1)
        cols = node_traffic(rng, twin, token0=1000 * t, p_noise=0.05 if t % 2 else 0.0)
        if t % 2 == 0:
            cols = steady(cols, twin)
        twin.submit_columns(**cols), dev.submit_columns(**cols)
        want = twin_step(twin, now)
        assert twin_hosting(twin, req, now) == res, t
        dev.step_node_begin(now, hosting=req, **KEPT)
        same_step(dev, dev.node_outbox(), want, f"request {t}")
        got = dev.node_hosting()
        assert got.pop("redone") == (want[0]["rows_general"] > 0)
        assert got == res, (t, got, res)
        same_engine(dev, twin, f"request {t}")


def test_small_rules():
    Gn, R = 300, 3
    V = np.arange(200, 230)
    dev, twin, rng = pair(Gn, R, seed=5, vacant=V)
    api, h = dev.api, dev._h

    def submit(t):
        cols = node_traffic(rng, twin, token0=1000 * t)
        twin.submit_columns(**cols), dev.submit_columns(**cols)

    def raw(groups=None, own=None, **kw):
        s = capi.GroupSet()
        if groups is not None:
            s.n, s.groups = len(groups), groups.ctypes.data
        if own is not None:
            s.self_slots = own.ctypes.data
        for k, v in kw.items():
            setattr(s, k, v)
        s.held = (groups, own)
        return s

    def begin(close=None, open_=None, f=FLAGS, handle=h):
        r = capi.NodeHostingRequest()
        r.close = C.addressof(close) if close is not None else None
        r.open = C.addressof(open_) if open_ is not None else None
        return api.step_node_hosted(handle, 100, f, None, None, None, C.byref(r))

    # before any view there is nothing to hand out
    with pytest.raises(EngineError):
        dev.node_hosting()
    v = capi.NodeHosting()
    assert api.node_hosting_view(h, C.byref(v)) == capi.EINVAL
    assert api.node_hosting_view(h, None) == capi.EINVAL and api.node_hosting_view(None, C.byref(v)) == capi.EINVAL
    # each refusal steps nothing and leaves the submitted rows queued: the next plain step delivers them as the twin's does
    submit(0)
    u32, u8 = (lambda *a: np.array(a, np.uint32)), (lambda *a: np.array(a, np.uint8))
    ok, vac = u32(1, 2, 3), u32(200, 201, 202)
    MAX = capi.NODE_HOSTING_MAX
    for what, kw in (("an index >= G, last", dict(close=raw(u32(1, 2, Gn)))), ("an index >= G, first", dict(open_=raw(u32(0xFFFFFFFF)))),
                     ("a range out of bounds", dict(close=raw(g0=Gn - 4, n=5))), ("a range that wraps", dict(open_=raw(g0=1, n=0xFFFFFFFF))),
                     ("JG_GROUPS_DEVICE", dict(close=raw(ok, flags=capi.GROUPS_DEVICE))),
                     ("JG_GROUPS_DEVICE on a range", dict(open_=raw(g0=200, n=5, flags=capi.GROUPS_DEVICE))),
                     ("an unknown flag", dict(close=raw(ok, flags=2))), ("an unknown high flag", dict(open_=raw(vac, flags=1 << 31))),
                     ("a list of JG_NODE_HOSTING_MAX + 1", dict(close=raw(np.zeros(MAX + 1, np.uint32)))),
                     ("not ascending", dict(close=raw(u32(1, 3, 2)))), ("a repeat", dict(open_=raw(u32(200, 200)))),
                     ("not ascending, the open", dict(close=raw(ok), open_=raw(u32(201, 200)))),
                     ("self_slots[i] >= R", dict(open_=raw(vac, u8(0, 1, R)))), ("self_slots[i] = 255", dict(open_=raw(vac, u8(255, 0, 0)))),
                     ("self_slots on the close set", dict(close=raw(ok, u8(0, 0, 0)))),
                     ("self_slots on a range of the close set", dict(close=raw(own=u8(0, 0, 0), g0=1, n=3))),
                     ("a good close and a bad open", dict(close=raw(ok), open_=raw(u32(Gn)))),
                     ("without JG_NODE_KEEP", dict(close=raw(ok), f=FLAGS & ~capi.NODE_KEEP)),
                     ("without JG_NODE_ASYNC", dict(close=raw(ok), f=FLAGS & ~capi.NODE_ASYNC)),
                     ("a plain step", dict(close=raw(ok), f=FLAGS & ~(capi.NODE_KEEP | capi.NODE_ASYNC))),
                     ("no handle", dict(close=raw(ok), handle=None))):
        assert begin(**kw) == capi.EINVAL, what
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.step_node_begin(100, hosting=dict(close=[1, 2]))
    with pytest.raises(EngineError):
        dev.step_node_begin(100, hosting=dict(close=[0, Gn]), **KEPT)
    with pytest.raises(EngineError):
        dev.step_node_begin(100, hosting=dict(self_slots=[0]), **KEPT)
    p = capi.Poll()
    p.want, p.g0, p.n = 32, 0, Gn  # a bad poll or a bad lookup refuses the hosted step too
    r = capi.NodeHostingRequest()
    assert api.step_node_hosted(h, 100, FLAGS, C.byref(p), None, None, C.byref(r)) == capi.EINVAL
    assert api.step_node_hosted(h, 100, FLAGS, None, None, C.byref(raw(u32(Gn))), C.byref(r)) == capi.EINVAL
    want = twin_step(twin, 100)
    same_step(dev, dev.step_node(100), want, "the plain step after the refusals")
    same_engine(dev, twin, "the plain step after the refusals")
    with pytest.raises(EngineError):
        dev.node_hosting()  # (a plain step is no kept step)
    # a range of any length beside a list with own slots (the engine's uniform one is 0); both sets NULL is attached and
    # writes nothing
    submit(1)
    dev.step_node_begin(100, hosting=dict(close=range(0, 150), open=[200, 205, 229], self_slots=[1, 0, 2]), **KEPT)
    first = twin_step(twin, 100)
    twin.close_groups(range(0, 150)), twin.open_groups([200, 205, 229], 100, self_slots=[1, 0, 2])
    # while it is outstanding the synchronous calls stay refused
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.open_groups([201], 100)
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.close_groups([160])
    submit(2)
    dev.step_node_begin(200, hosting=dict(), **KEPT)
    second = twin_step(twin, 200)
    same_step(dev, dev.node_outbox(), first, "the step with a range and own slots")
    got = dev.node_hosting()
    assert got == dict(NOTHING, redone=first[0]["rows_general"] > 0, closed=150, opened=3)
    assert dev.node_hosting() == got  # (the view may be asked again)
    same_step(dev, dev.node_outbox(), second, "the step with an empty request")
    assert api.node_hosting_view(h, C.byref(v)) == capi.OK
    assert (v.attached, v.state, v.closed, v.opened) == (1, capi.NODE_POLL_REDONE if second[0]["rows_general"] else 0, 0, 0)
    # nothing is outstanding: the synchronous calls work again, and the first dense tick after an open with a foreign own
    # slot is the twin's
    for e in (dev, twin):
        e.open_groups([201], 250), e.close_groups([160])
    same_engine(dev, twin, "the synchronous calls once the steps are viewed")
    submit(3)
    same_step(dev, dev.step_node(300), twin_step(twin, 300), "the dense tick after the foreign own slots")
    # empty sets are attached and write nothing; a kept step without a request views attached == 0
    submit(4)
    dev.step_node_begin(400, hosting=dict(close=[], open=range(0)), **KEPT)
    fourth = twin_step(twin, 400)
    submit(5)
    dev.step_node_begin(500, **KEPT)
    plain = twin_step(twin, 500)
    same_step(dev, dev.node_outbox(), fourth, "the step with empty sets")
    assert dev.node_hosting() == dict(NOTHING, redone=fourth[0]["rows_general"] > 0)
    same_step(dev, dev.node_outbox(), plain, "the kept step without a request")
    assert api.node_hosting_view(h, C.byref(v)) == capi.OK
    assert bytes(v) == bytes(C.sizeof(v))  # attached == 0 and everything else too
    assert dev.node_hosting() == {"redone": False}
    # hosting == NULL is exactly jg_step_node_looked; all NULL is jg_step_node
    submit(6)
    assert api.step_node_hosted(h, 600, FLAGS & ~(capi.NODE_ASYNC | capi.NODE_KEEP), None, None, None, None) == capi.OK
    same_step(dev, dev.node_outbox(), twin_step(twin, 600), "all NULL")
    same_engine(dev, twin, "at the end")


def test_small_the_callers_memory_is_free_on_return():
    """both sets, their lists and the own slots are copied at entry: through the C ABI alone, the arrays overwritten as soon
    as the call has returned - the step had general-path rows, so its passes are queued once more long after that"""
    V = np.arange(200, 230)
    dev, twin, rng = pair(seed=6, vacant=V)
    cols = rows_for([7, 8, 9])
    twin.submit_columns(**cols), dev.submit_columns(**cols)
    close, lst, own = np.arange(20, 120, dtype=np.uint32), np.array([200, 205, 229], np.uint32), np.array([1, 0, 2], np.uint8)
    sc, so, r = capi.GroupSet(), capi.GroupSet(), capi.NodeHostingRequest()
    sc.n, sc.groups = len(close), close.ctypes.data
    so.n, so.groups, so.self_slots = len(lst), lst.ctypes.data, own.ctypes.data
    r.close, r.open = C.addressof(sc), C.addressof(so)
    assert dev.api.step_node_hosted(dev._h, 100, FLAGS, None, None, None, C.byref(r)) == capi.OK
    close[:], lst[:], own[:] = 0xFFFFFFFF, 0xFFFFFFFF, 255
    C.memset(C.addressof(sc), 0xFF, C.sizeof(sc)), C.memset(C.addressof(so), 0xFF, C.sizeof(so)), C.memset(C.addressof(r), 0xFF, C.sizeof(r))
    want = twin_step(twin, 100)
    assert want[0]["rows_general"] > 0
    twin.close_groups(range(20, 120)), twin.open_groups([200, 205, 229], 100, self_slots=[1, 0, 2])
    same_step(dev, dev.node_outbox(), want, "the step begun through the C ABI")
    assert dev.node_hosting() == dict(NOTHING, redone=True, closed=100, opened=3)
    same_engine(dev, twin, "afterwards")


def test_a_list_of_the_most_entries():
    """JG_NODE_HOSTING_MAX listed entries are accepted in each set of one step"""
    MAX = capi.NODE_HOSTING_MAX
    Gn = 2 * MAX + 300
    dev, twin, rng = twin_pair(Gn, 3, seed=3)
    pick = np.random.default_rng(4)
    gone = np.sort(pick.choice(Gn, MAX + 100, replace=False))
    for e in (dev, twin):
        e.close_groups(gone)
    close = np.sort(pick.choice(twin.hosted_groups(), MAX, replace=False))
    cols = steady(node_traffic(rng, twin, p_noise=0.0, p_reorder=0.0), twin)
    twin.submit_columns(**cols), dev.submit_columns(**cols)
    want = twin_step(twin, 100)
    twin.close_groups(close), twin.open_groups(gone[:MAX], 100)
    dev.step_node_begin(100, hosting=dict(close=close, open=gone[:MAX]), **KEPT)
    same_step(dev, dev.node_outbox(), want, "the step of 2 x JG_NODE_HOSTING_MAX entries")
    assert dev.node_hosting() == dict(NOTHING, redone=False, closed=MAX, opened=MAX)
    same_engine(dev, twin, "afterwards")
    with pytest.raises(EngineError):
        dev.step_node_begin(200, hosting=dict(open=twin.vacant_groups()[:MAX + 1]), **KEPT)
