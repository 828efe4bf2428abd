"""Completions behind a kept node step (ABI v23): jg_step_node_awaited / jg_node_await_view - the completion feed with two
ticks in flight.

The awaited call defines no value of its own.  The reference is a TWIN, as in tests/test_node_poll.py: a second device
engine of the same seed and config, fed the same rows and stepped synchronously, then asked await_blocks(rows) and
watch_completions(...) with the step's request.  What node_completions() hands out for kept step t - begun with the same
request while step t - 1 was still outstanding - is that answer byte for byte (rows, total, stats), the step itself (its
outbox, its drains) is the twin's, and after the last tick one peek over the whole table is equal on both: no waiter was
registered twice or lost, and the order is the registration order.  The table holds 700 waiters and is kept between about
250 and 650: three tiles of the passes, the last one partial, the appends landing off tile boundaries.  The cases with
"small" in their ids also run on the emulated device (tests/test_node_await_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, capi
from josefine_amd.engine import EngineError
from node_step import compare_outboxes, node_traffic
from parity import compare_snapshots
from test_completion_feed import APPLIED, EXPIRED, LOST, same
from test_node_poll import DRAINS, EVERYTHING, steady, strip, twin_pair
from test_node_step import _same_rows
from test_poll import equal

pytestmark = pytest.mark.gpu

G = 1024 + 256 + 37
T = 40
CAPACITY = 700
LOW, HIGH = 250, 650  # the band the table is kept in: the waiters outstanding behind every registration
U = np.uint64

# per case: the watch of tick t (None: the step carries no request at all), and whether tick t registers
WATCH = {
    "all": lambda t: dict(stats=True),
    "limit7": lambda t: dict(limit=7, stats=True),
    "limit0": lambda t: dict(limit=0, stats=True),
    "peek": lambda t: dict(peek=t % 3 != 2, stats=True),
    "no-stats": lambda t: dict(limit=25),
    # watch-only ticks, register-only ticks (nothing is taken: counts only), kept steps without a request, and full ones
    "kinds": lambda t: (dict(stats=True), dict(stats=True), dict(limit=0), None)[t % 4],
    "with-poll": lambda t: dict(limit=60, stats=True),
}
REGISTERS = {"kinds": lambda t: t % 4 in (0, 2)}
SMALL = {("all", 3), ("limit7", 5), ("kinds", 3)}
CASES = [pytest.param(c, R, id=("small-" if (c, R) in SMALL else "") + f"{c}-{R}") for c in WATCH for R in (3, 5)]


def answer_equal(got, want, what):
    assert len(got) == len(want), what
    same(got[0], want[0], what)
    assert got[1] == want[1], (what, got[1], want[1])
    if len(want) == 3:
        assert got[2] == want[2], (what, got[2], want[2])


def waiters(rng, e, n, now, token0, far=0.0):
    """n waiters on the engine's state before the tick: ids around the heads (a share `far` of them far ahead: they wait),
    half of those on a leader guarded by its term - a leader deposed later loses them - and a third with a deadline
    around the coming ticks"""
    g = rng.integers(0, e.G, n)
    head, term = e.read("head").astype(np.int64)[g], e.read("term").astype(U)[g]
    ids = np.maximum(head + rng.integers(-2, 6, n), 1)
    ids = np.where(rng.random(n) < far, head + 10_000, ids)
    leads = e.read("role")[g] == capi.ROLE_LEADER
    guards = np.where(leads & (rng.random(n) < 0.5), term, 0).astype(U)
    deadlines = np.where(rng.random(n) < 0.3, np.maximum(now + rng.integers(-100, 600, n), 1), 0)
    deadlines = np.where(ids > head + 1000, 0, deadlines)  # (the far ones stay)
    return dict(groups=g, block_ids=ids, tokens=np.arange(n) + token0, terms=guards, deadlines_ms=deadlines)


def restarted(cols, groups):
    """the tick's rows and a Restart for each of `groups`: a leader comes back a follower (the reference's leader never steps
    down on a message), without a fault - what is guarded by its term is lost"""
    extra = dict(kind=np.full(len(groups), capi.CMD_RESTART, np.uint8), group=np.asarray(groups, np.uint32))
    return {k: (v if k.startswith("blk_") else np.concatenate([v, extra.get(k, np.zeros(len(groups), v.dtype))])) for k, v in cols.items()}


DEPOSE = (1, 4, 7)  # ticks that register guarded waiters on four leaders which the tick after restarts (both with general-path rows)


@pytest.mark.parametrize("case,R", CASES)
def test_awaited_steps_equal_the_twins_calls(case, R):
    """40 ticks of node_traffic, two steps in flight, the steps awaited as the case says: per tick the viewed outbox and the
    drains are the twin's and node_completions() is the twin's await_blocks + watch_completions after its synchronous step
    of that tick; ticks whose rows took the general path come back "redone", the others do not, and both kinds deliver."""
    watch, registers = WATCH[case], REGISTERS.get(case, lambda t: True)
    dev, twin, rng = twin_pair(G, R, seed=31 + R)
    pick = np.random.default_rng(5)  # (the waiters' own stream)
    for e in (dev, twin):
        e.open_waiters(CAPACITY)
    first = waiters(pick, twin, 400, 0, 1 << 40, far=0.7)  # registered synchronously: the first awaited step writes the head from it
    for e in (dev, twin):
        assert e.await_blocks(**first) == 400
    want = []  # per tick: the twin's outbox, drains, answers
    left = [400]  # the twin's table behind tick t - 1 (left[0]: before the first)
    begun = [0]  # rows registered by tick t - 1
    kinds = {True: [0, 0], False: [0, 0]}  # redone or not: ticks with a request, rows delivered
    states = set()
    token = 0
    deposed, waiting = None, 400

    def finish(t):
        b, drains, answer, polled, counts_only = want[t]
        a = dev.node_outbox()
        compare_outboxes(a, b, f"tick {t}")
        for fn in DRAINS:
            _same_rows(getattr(dev, fn)(), drains[fn], f"tick {t}: {fn}")
        got = dev.node_completions()
        if answer is None:
            assert got == {"redone": False}, t
        else:
            answer_equal(got["answer"], answer, f"tick {t}")
            assert got["redone"] == (b["rows_general"] > 0), (t, got["redone"], b["rows_general"])
            kinds[got["redone"]][0] += 1
            kinds[got["redone"]][1] += answer[1] if counts_only else len(answer[0])  # (limit=0 delivers its total)
            states.update(answer[0]["state"].tolist())
        if polled is not None:
            redone, p = strip(dev.node_poll())
            equal(p, polled, f"tick {t}: the poll")
            assert redone == (b["rows_general"] > 0)

    for t in range(T):
        now = 100 * (t + 1)
        cols = node_traffic(rng, twin, token0=1000 * t, p_noise=0.03 if t % 3 else 0.0, p_reorder=0.08 if t % 3 else 0.0)
        if t % 3 == 0:  # every third tick is all steady state: its chain is the one queued behind the step, not redone
            cols = steady(cols, twin)
        if deposed is not None:
            cols = restarted(cols, deposed)
            deposed = None
        w = watch(t)
        request = None
        if w is not None:
            # the library's bound: the table behind the newest VIEWED step (t - 2) and every row begun since (t - 1, t)
            bound = left[max(t - 1, 0)] + begun[t]
            room = min(CAPACITY - bound, HIGH - left[t])
            # (the traffic faults a few percent of the slots a tick and their waiters are lost: the table is topped up)
            n = int(pick.integers(20, 70) + max(0, 500 - waiting)) if registers(t) else 0
            n = max(0, min(n, room))
            far = 0.8 if waiting < 500 else 0.1
            new = waiters(pick, twin, n, now, token, far=far) if n else {}
            if t in DEPOSE and n >= 4:
                deposed = np.nonzero((twin.read("role") == capi.ROLE_LEADER) & (twin.read("fault") == 0))[0][-4:]
                assert len(deposed) == 4
                new["groups"][:4], new["block_ids"][:4] = deposed, twin.read("head")[deposed].astype(np.int64) + 10_000
                new["terms"][:4], new["deadlines_ms"][:4] = twin.read("term")[deposed].astype(U), 0
            request = dict(new, now_ms=now, **w)
            token += n
        twin.submit_columns(**cols)
        b = twin.step_node(now)
        drains = {fn: getattr(twin, fn)() for fn in DRAINS}
        answer = None
        if request is not None:
            reg = {k: request[k] for k in ("groups", "block_ids", "tokens", "terms", "deadlines_ms") if k in request}
            if reg:
                assert twin.await_blocks(**reg) == len(reg["groups"])
            if reg:  # (the band is the table's size where an append lands)
                assert LOW <= len(reg["groups"]) + left[t] <= HIGH, (t, left)
            answer = twin.watch_completions(now, w.get("limit"), w.get("peek", False), stats=w.get("stats", False))
        poll = dict(EVERYTHING) if case == "with-poll" else None
        want.append((b, drains, answer, twin.poll(**poll) if poll else None, bool(w) and w.get("limit") == 0))
        begun.append(len(request.get("groups", ())) if request else 0)
        s = twin.watch_completions(now, limit=0, peek=True, stats=True)[2]
        left.append(s["left"])
        waiting = s["waiting"]  # (of them: not done by now)
        dev.submit_columns(**cols)
        dev.step_node_begin(now, async_=True, keep=True, poll=poll, completions=request)
        if t % 9 == 4:  # a read between begin and view settles the newest step; the answer is what it would have been
            compare_snapshots(dev, twin, f"tick {t}, read while it is outstanding")
        if t:
            finish(t - 1)
    finish(T - 1)
    compare_snapshots(dev, twin, "after the last tick")
    # nothing is outstanding: the synchronous calls again, on the one table - every waiter once, in registration order
    x, y = (e.watch_completions(100 * T, peek=True, stats=True) for e in (dev, twin))
    answer_equal(x, y, "a peek over the whole table afterwards")
    x, y = (e.watch_completions(2**64 - 2, stats=True) for e in (dev, twin))
    answer_equal(x, y, "the end of time afterwards")
    assert x[2]["left"] == left[-1] - len(x[0])
    for redone in (True, False):
        assert kinds[redone][0] >= 5 and kinds[redone][1] >= 1, kinds
    if case == "all":  # (plain LOST: a guard whose leader was deposed)
        assert {APPLIED, LOST, EXPIRED} <= states, states


def test_small_rules():
    Gn, R = 300, 3
    dev, twin, rng = twin_pair(Gn, R, seed=5)
    api, h = dev.api, dev._h
    kept = dict(async_=True, keep=True)
    flags = capi.NODE_LEADER_HALF | capi.NODE_FOLLOWER_HALF | capi.NODE_TICK | capi.NODE_ASYNC | capi.NODE_KEEP

    def submit(t):
        cols = node_traffic(rng, twin, token0=1000 * t)
        twin.submit_columns(**cols), dev.submit_columns(**cols)

    def same_step(a, now, what):
        compare_outboxes(a, twin.step_node(now), what)
        for fn in DRAINS:
            _same_rows(getattr(dev, fn)(), getattr(twin, fn)(), f"{what}: {fn}")

    def rows_of(n, **kw):
        r = np.zeros(n, capi.AWAIT_ROW_DTYPE)
        r["group"], r["block_id"], r["token"] = np.arange(n) % Gn, 1 << 40, np.arange(n) + 500
        for k, v in kw.items():
            r[k][-1:] = v
        return r

    def raw(r=None, **kw):
        q = capi.NodeAwaitRequest()
        q.rows, q.n = (r.ctypes.data, len(r)) if r is not None and len(r) else (None, 0)
        q.cap = 8
        for k, v in kw.items():
            setattr(q, k, v)
        q.held = r
        return q

    begin = lambda q, f=flags: api.step_node_awaited(h, 100, f, None, C.byref(q))  # noqa: E731

    # before any view there is nothing to hand out
    with pytest.raises(EngineError):
        dev.node_completions()
    v = capi.NodeAwait()
    assert api.node_await_view(h, C.byref(v)) == capi.EINVAL
    assert api.node_await_view(h, None) == capi.EINVAL and api.node_await_view(None, C.byref(v)) == capi.EINVAL
    # each refusal steps nothing and leaves the submitted rows queued: the next plain step delivers them as the twin's does
    submit(0)
    assert begin(raw(rows_of(2))) == capi.EINVAL  # no open table
    for e in (dev, twin):
        e.open_waiters(10)
    for what, q in (("group out of range", raw(rows_of(3, group=Gn))), ("flags", raw(rows_of(3, flags=1))),
                    ("reserved", raw(rows_of(3, reserved=1))), ("block id 0", raw(rows_of(3, block_id=0))),
                    ("an unknown watch flag", raw(rows_of(1), flags=2)), ("the clock's one refused value", raw(rows_of(1), now_ms=2**64 - 1)),
                    ("null rows", raw(None, n=2)), ("want_stats", raw(rows_of(1), want_stats=2))):
        assert begin(q) == capi.EINVAL, what
    assert begin(raw(rows_of(11))) == capi.ECAPACITY
    assert begin(raw(rows_of(1)), flags & ~capi.NODE_KEEP) == capi.EINVAL  # a request travels with a kept step
    assert begin(raw(rows_of(1)), flags & ~(capi.NODE_KEEP | capi.NODE_ASYNC)) == capi.EINVAL
    assert api.step_node_awaited(None, 100, flags, None, C.byref(raw(rows_of(1)))) == capi.EINVAL
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.step_node_begin(100, completions=dict(now_ms=100))
    p = capi.Poll()
    p.want, p.g0, p.n = 32, 0, Gn  # a bad poll refuses the awaited step too
    assert api.step_node_awaited(h, 100, flags, C.byref(p), C.byref(raw(rows_of(1)))) == capi.EINVAL
    same_step(dev.step_node(100), 100, "the plain step after the refusals")
    compare_snapshots(dev, twin, "the plain step after the refusals")
    with pytest.raises(EngineError):
        dev.node_completions()  # (a plain step is no kept step)
    # an empty table: a watch-only step on it answers zeros, and leaves it empty
    submit(1)
    dev.step_node_begin(200, completions=dict(now_ms=200, stats=True), **kept)
    first = twin.step_node(200), {fn: getattr(twin, fn)() for fn in DRAINS}, twin.watch_completions(200, stats=True)
    assert first[2][1] == 0 and first[2][2]["left"] == 0
    # while it is outstanding the three synchronous calls stay refused
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.watch_completions()
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.await_blocks([1], [1], [1])
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.open_waiters(20)
    # the capacity bound: 6 rows with the second step, then 5 more are refused by the bound ...
    submit(2)
    done_at = np.nonzero(twin.read("commit") >= 2)[0][:3]  # (block 1 is applied there whatever the role; a slot that is closed or faulted loses it: done too)
    assert len(done_at) == 3
    six = dict(groups=np.concatenate([done_at, np.arange(3)]), block_ids=[1, 1, 1] + [1 << 40] * 3, tokens=np.arange(6) + 100, now_ms=300, stats=True)
    dev.step_node_begin(300, completions=six, **kept)
    second = twin.step_node(300), {fn: getattr(twin, fn)() for fn in DRAINS}
    assert twin.await_blocks(six["groups"], six["block_ids"], six["tokens"]) == 6
    second += (twin.watch_completions(300, stats=True),)
    removed = len(second[2][0])
    assert 0 < removed < 6  # a condition of the test: the view lowers the bound, and something stays
    compare_outboxes(dev.node_outbox(), first[0], "the step on the empty table")
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), first[1][fn], f"the step on the empty table: {fn}")
    got = dev.node_completions()
    answer_equal(got["answer"], first[2], "the step on the empty table")
    five = raw(rows_of(5), now_ms=400, want_stats=1)
    submit(3)
    assert api.step_node_awaited(h, 400, flags, None, C.byref(five)) == capi.ECAPACITY  # 6 + 5 > 10: the second step's watch is not viewed
    compare_outboxes(dev.node_outbox(), second[0], "the step that registered six")
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), second[1][fn], f"the step that registered six: {fn}")
    got = dev.node_completions()
    answer_equal(got["answer"], second[2], "the step that registered six")
    assert got["redone"] == (second[0]["rows_general"] > 0)
    assert dev.node_completions()["answer"][1] == second[2][1]  # (the view may be asked again)
    # ... and the same call is accepted after the view that lowers it (6 - removed + 5 <= 10)
    assert api.step_node_awaited(h, 400, flags, None, C.byref(five)) == capi.OK
    dev._kept_backlog.append(False), dev._kept_await.append((True, True))  # (the mirror's note of the step begun behind its back)
    dev._await_n += 5
    third = twin.step_node(400), {fn: getattr(twin, fn)() for fn in DRAINS}
    r = five.held
    assert twin.await_blocks(r["group"], r["block_id"], r["token"]) == 5
    third += (twin.watch_completions(400, limit=8, stats=True),)
    # a kept step without a request leaves the table alone and views attached == 0
    submit(4)
    dev.step_node_begin(500, **kept)
    plain = twin.step_node(500), {fn: getattr(twin, fn)() for fn in DRAINS}
    compare_outboxes(dev.node_outbox(), third[0], "the third step")
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), third[1][fn], f"the third step: {fn}")
    answer_equal(dev.node_completions()["answer"], third[2], "the third step")
    compare_outboxes(dev.node_outbox(), plain[0], "the kept step without a request")
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), plain[1][fn], f"the kept step without a request: {fn}")
    assert api.node_await_view(h, C.byref(v)) == capi.OK
    assert bytes(v) == bytes(C.sizeof(v))  # attached == 0 and everything else too
    assert dev.node_completions() == {"redone": False}
    # nothing is outstanding: the three synchronous calls work again, on the table the awaited steps left
    assert api.engine_await_open(h, 0) == capi.EINVAL  # waiters are outstanding
    answer_equal(dev.watch_completions(500, peek=True, stats=True), twin.watch_completions(500, peek=True, stats=True), "afterwards")
    for e in (dev, twin):
        assert e.await_blocks([3], [1 << 41], [77]) == 1
    # ... mixed with awaited steps: the next one writes the head from the host's values
    submit(5)
    dev.step_node_begin(600, completions=dict(now_ms=2**64 - 2, stats=True), **kept)
    last = twin.step_node(600), twin.watch_completions(2**64 - 2, stats=True)
    compare_outboxes(dev.node_outbox(), last[0], "the last step")
    answer_equal(dev.node_completions()["answer"], last[1], "the last step")
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), getattr(twin, fn)(), f"the last step: {fn}")
    x, y = dev.watch_completions(2**64 - 2, stats=True), twin.watch_completions(2**64 - 2, stats=True)
    answer_equal(x, y, "at the end")
    # await == NULL is exactly jg_step_node_polled; both NULL is jg_step_node
    submit(6)
    assert api.step_node_awaited(h, 700, flags & ~(capi.NODE_ASYNC | capi.NODE_KEEP), None, None) == capi.OK
    compare_outboxes(dev.node_outbox(), twin.step_node(700), "both NULL")
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), getattr(twin, fn)(), f"both NULL: {fn}")
    compare_snapshots(dev, twin, "at the end")
    if x[2]["left"] == 0:
        dev.open_waiters(0)
