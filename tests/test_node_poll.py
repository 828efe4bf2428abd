"""A poll behind a kept node step (ABI v21): jg_step_node_polled / jg_node_poll_view - the feeds with two ticks in flight.

The polled call defines no value of its own.  The reference is a TWIN, as in tests/test_poll.py: a second device engine of
the same seed and config, fed the same rows and stepped synchronously (submit_columns, then step_node(now)), then asked
poll(**request).  What node_poll() hands out for kept step t - begun with the same request while step t - 1 was still
outstanding - is that answer byte for byte, and the step itself (its outbox, its drains) is the twin's: the poll disturbs
nothing.  The cases with "small" in their ids also run on the emulated device (tests/test_node_poll_emulated.py)."""
import numpy as np
import pytest

from josefine_amd import BatchedRaft, capi
from josefine_amd.engine import EngineError
from node_step import classify, compare_outboxes, node_traffic
from parity import compare_snapshots
from test_node_step import _same_rows, mixed_pair
from test_poll import LAGS, equal

pytestmark = pytest.mark.gpu

G = 1024 + 256 + 37  # two tiles of the poll passes: the second with one full row and a 37-lane partial wave
T = 40
DRAINS = ("drain_messages", "drain_applies", "drain_faults")
EVERYTHING = dict(leaders={}, replicas=dict(LAGS), commits=dict(backlog=True), census=True, repl_census=1)
CLOCK = dict(max_behind_ms=250, caught_lag=0, join_lag=0)  # the time rule: a member may be behind for two and a half ticks


REQUESTS = {
    "everything": lambda t: dict(EVERYTHING),
    "leaders": lambda t: dict(leaders={}),
    "replicas": lambda t: dict(replicas=dict(LAGS)),
    "commits": lambda t: dict(commits=dict(backlog=True)),
    "range": lambda t: dict(EVERYTHING, g0=5, n=G - 9),
    "limit7": lambda t: dict(leaders=dict(limit=7), replicas=dict(LAGS, limit=7), commits=dict(limit=7, backlog=True), census=True,
                                   repl_census=1),
    "peek-leaders": lambda t: dict(EVERYTHING, leaders=dict(peek=t % 3 != 2)),
    "peek-replicas": lambda t: dict(EVERYTHING, replicas=dict(LAGS, peek=t % 3 != 2)),
    "peek-commits": lambda t: dict(EVERYTHING, commits=dict(backlog=True, peek=t % 3 != 2)),
    "commits-only": lambda t: dict(EVERYTHING, commits=dict(commits_only=True, backlog=True, limit=400)),
    "timed": lambda t: dict(EVERYTHING, replicas=dict(CLOCK, now_ms=100 * (t + 1), limit=300)),
}
# the cases that fit the emulated device (tests/test_node_poll_emulated.py), and every case at both replica counts
SMALL = {("everything", 3), ("limit7", 5), ("timed", 3)}
CASES = [pytest.param(c, R, id=("small-" if (c, R) in SMALL else "") + f"{c}-{R}") for c in REQUESTS for R in (3, 5)]
SILENT = range(8, 22)  # the ticks of the timed case in which one follower of every partition says nothing


def silence(cols, node_id):
    """the tick's rows without the AppendResponses of member `node_id` (no such row owns blocks)"""
    keep = ~((cols["kind"] == capi.CMD_APPEND_RESPONSE) & (cols["from_"] == node_id))
    return {k: (v if k.startswith("blk_") else v[keep]) for k, v in cols.items()}


def steady(cols, e):
    """the tick's rows of the partitions that stay in column form: no row of such a tick takes the general path (the blocks
    of the rows left out stay in the batch, unreferenced)"""
    general = classify(cols, e.read("role"), e.read("self_slot"), e.node_ids)
    keep = ~general[cols["group"]]
    return {k: (v if k.startswith("blk_") else v[keep]) for k, v in cols.items()}


def twin_pair(Gn, R, seed):
    return mixed_pair(BatchedRaft, BatchedRaft, Gn, R, seed=seed, election_timeout_ms=(700, 1500))


def strip(answer):
    answer = dict(answer)
    return answer.pop("redone"), answer


def totals(answer):
    return sum(answer[k][1] for k in ("leaders", "replicas", "commits") if k in answer)


@pytest.mark.parametrize("case,R", CASES)
def test_polled_steps_equal_the_twins_polls(case, R):
    """40 ticks of node_traffic, two steps in flight, every step polled: per tick the viewed outbox and the drains are the
    twin's, and node_poll() is the twin's poll(**request) after its synchronous step of that tick; afterwards one poll of
    everything is equal on both - the shadows and the clocks advanced identically.  Ticks whose rows took the general path come
    back "redone" (the poll ran behind the catch-up pass), the others do not, and both kinds report changes."""
    request = REQUESTS[case]
    dev, twin, rng = twin_pair(G, R, seed=77 + R)
    quiet_id = int(twin.node_ids[(int(twin.read("self_slot")[0]) + 1) % R])
    want = []  # per tick: the twin's outbox, drains and poll
    kinds = {True: [0, 0], False: [0, 0]}  # redone or not: ticks, ticks with a nonzero feed total

    def finish(t):
        b, drains, polled = want[t]
        a = dev.node_outbox()
        compare_outboxes(a, b, f"tick {t}")
        for fn in DRAINS:
            _same_rows(getattr(dev, fn)(), drains[fn], f"tick {t}: {fn}")
        redone, got = strip(dev.node_poll())
        equal(got, polled, f"tick {t}")
        assert redone == (b["rows_general"] > 0), (t, redone, b["rows_general"])
        kinds[redone][0] += 1
        kinds[redone][1] += totals(polled) > 0

    for t in range(T):
        now = 100 * (t + 1)
        cols = node_traffic(rng, twin, token0=1000 * t, p_noise=0.03 if t % 3 else 0.0, p_reorder=0.08 if t % 3 else 0.0)
        if case == "timed" and t in SILENT:
            cols = silence(cols, quiet_id)
        if t % 3 == 0:  # every third tick is all steady state: its poll is the one queued behind the step, not redone
            cols = steady(cols, twin)
        twin.submit_columns(**cols)
        b = twin.step_node(now)
        want.append((b, {fn: getattr(twin, fn)() for fn in DRAINS}, twin.poll(**request(t))))
        dev.submit_columns(**cols)
        dev.step_node_begin(now, async_=True, keep=True, poll=request(t))
        if t % 9 == 4:  # a read between begin and view settles the newest step; the poll's answer is what it would have been
            compare_snapshots(dev, twin, f"tick {t}, read while it is outstanding")
        if t:
            finish(t - 1)
    finish(T - 1)
    compare_snapshots(dev, twin, "after the last tick")
    last = dict(EVERYTHING, replicas=dict(CLOCK, now_ms=100 * (T + 1))) if case == "timed" else EVERYTHING
    equal(dev.poll(**last), twin.poll(**last), "one poll of everything afterwards")
    for redone in (True, False):
        assert kinds[redone][0] >= 5 and kinds[redone][1] >= 1, kinds


def test_small_rules():
    Gn, R = 300, 3
    dev, twin, rng = twin_pair(Gn, R, seed=5)
    api, h = dev.api, dev._h

    def submit(t):
        cols = node_traffic(rng, twin, token0=1000 * t)
        twin.submit_columns(**cols), dev.submit_columns(**cols)

    def same_step(a, what):
        compare_outboxes(a, twin.step_node(100), what)
        for fn in DRAINS:
            _same_rows(getattr(dev, fn)(), getattr(twin, fn)(), f"{what}: {fn}")

    # before any view there is nothing to hand out
    with pytest.raises(EngineError):
        dev.node_poll()
    # a refused call steps nothing and leaves the submitted rows queued: the next plain step delivers them as the twin's does
    submit(0)
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.step_node_begin(100, poll=dict(EVERYTHING))  # a poll travels with a kept step
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.step_node_begin(100, async_=True, poll=dict(EVERYTHING))
    kept = dict(async_=True, keep=True)

    def raw(**kw):
        p = capi.Poll()
        p.want, p.g0, p.n = 31, 0, Gn
        p.policy = capi.IsrPolicy(2, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    import ctypes as C
    flags = capi.NODE_LEADER_HALF | capi.NODE_FOLLOWER_HALF | capi.NODE_TICK | capi.NODE_ASYNC | capi.NODE_KEEP
    clock = capi.IsrClock(2 ** 64 - 1, 100, 0, 0)
    for what, p in (("an unknown want bit", raw(want=32 | 7)), ("want 0", raw(want=0)), ("join_lag above leave_lag", raw(policy=capi.IsrPolicy(1, 2))),
                    ("a range out of bounds", raw(g0=1, n=Gn)), ("now_ms == UINT64_MAX", raw(clock=C.pointer(clock))),
                    ("an unknown commit flag", raw(commit_flags=4))):
        assert api.step_node_polled(h, 100, flags, C.byref(p)) == capi.EINVAL, what
    with pytest.raises(EngineError):
        dev.step_node_begin(100, poll=dict(leaders={}, g0=Gn - 3, n=4), **kept)
    same_step(dev.step_node(100), "the plain step after the refusals")
    compare_snapshots(dev, twin, "the plain step after the refusals")
    with pytest.raises(EngineError):
        dev.node_poll()  # (a plain step is no kept step)
    # the output pointers of the request are never written through, the backlog pointer only says that it is wanted
    submit(1)
    p = raw(leaders_cap=Gn, replicas_cap=Gn, commits_cap=Gn, census_lag_limit=1)
    p.leaders = p.replicas = p.commits = 8  # (no memory there)
    p.backlog = C.cast(8, C.POINTER(capi.CommitBacklog))
    assert api.step_node_polled(h, 200, flags, C.byref(p)) == capi.OK
    dev._kept_backlog = [True]  # (the mirror's note of the step begun behind its back: its backlog is wanted)
    polled = twin.step_node(200), {fn: getattr(twin, fn)() for fn in DRAINS}, twin.poll(**EVERYTHING)
    # ... and while it is outstanding the synchronous poll stays refused
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.poll(**EVERYTHING)
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.watch_leaders()
    # a kept step without a request leaves the feeds alone and views want == 0
    submit(2)
    dev.step_node_begin(300, **kept)
    plain = twin.step_node(300), {fn: getattr(twin, fn)() for fn in DRAINS}
    compare_outboxes(dev.node_outbox(), polled[0], "the polled step")
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), polled[1][fn], f"the polled step: {fn}")
    redone, got = strip(dev.node_poll())
    equal(got, polled[2], "the polled step")
    assert redone == (polled[0]["rows_general"] > 0)
    assert strip(dev.node_poll())[1].keys() == got.keys()  # (the view may be asked again)
    compare_outboxes(dev.node_outbox(), plain[0], "the kept step without a poll")
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), plain[1][fn], f"the kept step without a poll: {fn}")
    v = capi.NodePoll()
    assert api.node_poll_view(h, C.byref(v)) == capi.OK
    assert bytes(v) == bytes(C.sizeof(v))  # want == 0 and everything else too
    assert dev.node_poll() == {"redone": False}
    # nothing is outstanding: the synchronous poll works again, on the shadows the polled step advanced
    equal(dev.poll(**EVERYTHING), twin.poll(**EVERYTHING), "a poll once the steps are viewed")
    # null arguments
    assert api.node_poll_view(h, None) == capi.EINVAL and api.node_poll_view(None, C.byref(v)) == capi.EINVAL
    assert api.step_node_polled(None, 100, flags, C.byref(raw())) == capi.EINVAL
    # request == NULL is exactly jg_step_node
    submit(3)
    assert api.step_node_polled(h, 400, flags & ~(capi.NODE_ASYNC | capi.NODE_KEEP), None) == capi.OK
    compare_outboxes(dev.node_outbox(), twin.step_node(400), "request == NULL")
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), getattr(twin, fn)(), f"request == NULL: {fn}")
    compare_snapshots(dev, twin, "at the end")
    equal(dev.poll(**EVERYTHING), twin.poll(**EVERYTHING), "at the end")


def test_small_polls_and_polled_steps_mix():
    """once nothing is outstanding jg_engine_poll and the separate feed calls may be mixed with polled steps: one set of shadows
    and clocks - and a read between begin and view settles the step without changing the poll's answer"""
    Gn, R = 300, 3
    dev, twin, rng = twin_pair(Gn, R, seed=9)
    half = dict(leaders=dict(limit=40), replicas=dict(CLOCK, now_ms=0, limit=40), commits=dict(limit=40, backlog=True))
    for t in range(6):
        now = 100 * (t + 1)
        req = dict(half, replicas=dict(half["replicas"], now_ms=now))
        cols = node_traffic(rng, twin, token0=1000 * t)
        twin.submit_columns(**cols), dev.submit_columns(**cols)
        b = twin.step_node(now)
        drains = {fn: getattr(twin, fn)() for fn in DRAINS}
        polled = twin.poll(**req)
        dev.step_node_begin(now, async_=True, keep=True, poll=req)
        assert dev.read("commit").tobytes() == twin.read("commit").tobytes()  # (settles the step)
        compare_outboxes(dev.node_outbox(), b, f"tick {t}")
        for fn in DRAINS:
            _same_rows(getattr(dev, fn)(), drains[fn], f"tick {t}: {fn}")
        redone, got = strip(dev.node_poll())
        equal(got, polled, f"tick {t}")
        assert redone == (b["rows_general"] > 0)
        if t % 2:  # nothing is outstanding: the separate calls take what the small caps left
            for e in (dev, twin):
                e.answers = e.watch_leaders(limit=25), e.watch_commits(limit=25), e.watch_replicas_timed(now, 250, limit=25, peek=True)
            for x, y in zip(dev.answers, twin.answers):
                assert x[1] == y[1] and x[0].tobytes() == y[0].tobytes(), t
