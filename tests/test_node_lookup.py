"""Point queries behind a kept node step (ABI v25): jg_step_node_looked / jg_node_lookup_view - the state of exactly these
partitions with two ticks in flight.

The looked call defines no value of its own.  The reference is a TWIN, as in tests/test_node_poll.py and
tests/test_node_await.py: a second device engine of the same seed and config, fed the same rows and stepped synchronously,
then asked lookup(...) with the step's set.  What node_lookup() hands out for kept step t - begun with the same set while
step t - 1 was still outstanding - is that answer byte for byte (rows and progress heads), and the step itself (its
outbox, its drains, its poll, its completions) is the twin's: the lookup disturbs nothing.  The decode's rare branches are
compared once over the world of tests/test_lookup_groups.py.  The cases with "small" in their ids also run on the emulated
device (tests/test_node_lookup_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import capi
from josefine_amd.engine import EngineError
from node_step import compare_outboxes, node_traffic
from parity import compare_snapshots
from test_lookup_groups import STATES, same, world
from test_node_await import answer_equal, waiters
from test_node_poll import DRAINS, EVERYTHING, steady, strip, twin_pair
from test_node_step import _same_rows
from test_poll import equal

pytestmark = pytest.mark.gpu

G = 1024 + 256 + 37
LENGTHS = (0, 1, 63, 64, 65, 257)  # around a wave, and more than one workgroup with a partial last one


def shape(t, rng, Gn):
    """the lookup of tick t: the list lengths, a shuffled list with repeats and the range form that ends at G, cycling; each
    of them with and without the progress heads as the ticks go round"""
    k = t % 8
    progress = (t // 8 + k) % 2 == 1
    if k < len(LENGTHS):
        return dict(groups=rng.integers(0, Gn, LENGTHS[k]), progress=progress)
    if k == 6:
        return dict(groups=rng.permutation(np.concatenate([rng.integers(0, Gn, 90)] * 2 + [np.arange(Gn - 20, Gn)])), progress=progress)
    return dict(g0=Gn - 201, progress=progress)  # (n: up to G)


def lookup_equal(got, want, progress, what):
    rows, match = want if progress else (want, None)
    same(got["rows"], rows, what)
    assert ("match" in got) == progress, what
    if progress:
        assert got["match"].shape == match.shape and got["match"].tobytes() == match.tobytes(), what


# (case, R, ticks): the cases with "small" in their ids are R in {3, 5}, lists of at most 257 entries and 6 ticks
CASES = [pytest.param("lookup", 3, 6, id="small-3"), pytest.param("lookup", 5, 6, id="small-5"),
         pytest.param("lookup", 3, 24, id="lookup-3"), pytest.param("lookup", 5, 24, id="lookup-5"), pytest.param("lookup", 8, 24, id="lookup-8"),
         pytest.param("with-poll-and-completions", 3, 24, id="with-poll-and-completions-3")]


@pytest.mark.parametrize("case,R,T", CASES)
def test_looked_steps_equal_the_twins_lookups(case, R, T):
    """T ticks of node_traffic, two steps in flight, every step looked: per tick the viewed outbox and the drains are the
    twin's and node_lookup() is the twin's lookup(...) after its synchronous step of that tick; ticks whose rows took the
    general path come back "redone", the others do not, and both kinds deliver rows.  One case carries a poll and a
    completion request on the same steps: all three answers are the twin's."""
    dev, twin, rng = twin_pair(G, R, seed=53 + R)
    pick = np.random.default_rng(11)  # (the lists' and the waiters' own stream)
    full = case == "with-poll-and-completions"
    if full:
        for e in (dev, twin):
            e.open_waiters(700)
    want = []
    kinds = {True: [0, 0], False: [0, 0]}  # redone or not: ticks, rows delivered
    token = 0

    def finish(t):
        b, drains, looked, progress, polled, answer = want[t]
        compare_outboxes(dev.node_outbox(), b, f"tick {t}")
        for fn in DRAINS:
            _same_rows(getattr(dev, fn)(), drains[fn], f"tick {t}: {fn}")
        got = dev.node_lookup()
        lookup_equal(got, looked, progress, f"tick {t}")
        assert got["redone"] == (b["rows_general"] > 0), (t, got["redone"], b["rows_general"])
        kinds[got["redone"]][0] += 1
        kinds[got["redone"]][1] += len(got["rows"])
        if full:
            redone, p = strip(dev.node_poll())
            equal(p, polled, f"tick {t}: the poll")
            done = dev.node_completions()
            answer_equal(done["answer"], answer, f"tick {t}: the completions")
            assert redone == done["redone"] == got["redone"]
        else:
            assert dev.node_poll() == {"redone": False} and dev.node_completions() == {"redone": False}

    for t in range(T):
        now = 100 * (t + 1)
        cols = node_traffic(rng, twin, token0=1000 * t, p_noise=0.03 if t % 3 else 0.0, p_reorder=0.08 if t % 3 else 0.0)
        if t % 3 == 0:  # every third tick is all steady state: its lookup is the one queued behind the step, not redone
            cols = steady(cols, twin)
        look = shape(t, pick, G)
        poll = dict(EVERYTHING) if full else None
        request = None
        if full:
            new = waiters(pick, twin, 20, now, token, far=0.5)
            token += 20
            request = dict(new, now_ms=now, stats=True)
        twin.submit_columns(**cols)
        b = twin.step_node(now)
        drains = {fn: getattr(twin, fn)() for fn in DRAINS}
        polled = answer = None
        if full:
            polled = twin.poll(**poll)
            assert twin.await_blocks(**new) == 20
            answer = twin.watch_completions(now, stats=True)
        want.append((b, drains, twin.lookup(**look), look["progress"], polled, answer))
        dev.submit_columns(**cols)
        dev.step_node_begin(now, async_=True, keep=True, poll=poll, completions=request, lookup=look)
        if t % 9 == 4:  # a read between begin and view settles the newest step; the answer is what it would have been
            compare_snapshots(dev, twin, f"tick {t}, read while it is outstanding")
        if t:
            finish(t - 1)
    finish(T - 1)
    compare_snapshots(dev, twin, "after the last tick")
    same(dev.lookup(), twin.lookup(), "a lookup of everything afterwards")
    for redone in (True, False):
        assert kinds[redone][0] >= 2 and kinds[redone][1] >= 1, kinds


@pytest.mark.parametrize("R", [pytest.param(5, id="small-world-5"), pytest.param(3, id="small-world-3")])
def test_the_decodes_rare_branches_behind_a_kept_step(R):
    """the world of tests/test_lookup_groups.py - leaders with escaped lag fields, candidates, queued requests, faulted and
    vacant slots - built twice more (the cached one stays as the other tests expect it): all 300 slots looked up behind a
    kept step that changes nothing, so that every one of STATES is among the slots compared, and behind one that ticks"""
    dev, twin = world.__wrapped__(R), world.__wrapped__(R)
    missing = [k for k in STATES if not twin.states[k].any()]
    assert not missing, missing
    lst = np.random.default_rng(R).permutation(twin.G)
    for tick, now in ((False, 4400), (True, 9000)):
        b = twin.e.step_node(now, tick=tick)
        drains = {fn: getattr(twin.e, fn)() for fn in DRAINS}
        rows, match = twin.e.lookup(lst, progress=True)
        if not tick:  # a condition of the test: the step left the world as it was built, every state is still there
            same(rows, twin.rows[lst], "the twin behind the step that changes nothing")
            assert match.tobytes() == twin.match[lst].tobytes()
        dev.e.step_node_begin(now, tick=tick, async_=True, keep=True, lookup=dict(groups=lst, progress=True))
        compare_outboxes(dev.e.node_outbox(), b, f"tick={tick}")
        for fn in DRAINS:
            _same_rows(getattr(dev.e, fn)(), drains[fn], f"tick={tick}: {fn}")
        lookup_equal(dev.e.node_lookup(), (rows, match), True, f"tick={tick}")
    compare_snapshots(dev.e, twin.e, "afterwards")


def test_small_rules():
    Gn, R = 300, 3
    dev, twin, rng = twin_pair(Gn, R, seed=5)
    api, h = dev.api, dev._h
    kept = dict(async_=True, keep=True)
    flags = capi.NODE_LEADER_HALF | capi.NODE_FOLLOWER_HALF | capi.NODE_TICK | capi.NODE_ASYNC | capi.NODE_KEEP
    MAX = capi.NODE_LOOKUP_MAX

    def submit(t):
        cols = node_traffic(rng, twin, token0=1000 * t)
        twin.submit_columns(**cols), dev.submit_columns(**cols)

    def twin_step(now):
        return twin.step_node(now), {fn: getattr(twin, fn)() for fn in DRAINS}

    def same_step(a, want, what):
        compare_outboxes(a, want[0], what)
        for fn in DRAINS:
            _same_rows(getattr(dev, fn)(), want[1][fn], f"{what}: {fn}")

    def raw(groups=None, **kw):
        s = capi.GroupSet()
        if groups is not None:
            s.n, s.groups = len(groups), groups.ctypes.data
        for k, v in kw.items():
            setattr(s, k, v)
        s.held = groups
        return s

    begin = lambda s, f=flags: api.step_node_looked(h, 100, f, None, None, C.byref(s))  # noqa: E731

    # before any view there is nothing to hand out
    with pytest.raises(EngineError):
        dev.node_lookup()
    v = capi.NodeLookup()
    assert api.node_lookup_view(h, C.byref(v)) == capi.EINVAL
    assert api.node_lookup_view(h, None) == capi.EINVAL and api.node_lookup_view(None, C.byref(v)) == capi.EINVAL
    # each refusal steps nothing and leaves the submitted rows queued: the next plain step delivers them as the twin's does
    submit(0)
    ok = np.arange(5, dtype=np.uint32)
    bad_last, bad_first = ok.copy(), ok.copy()
    bad_last[-1], bad_first[0] = Gn, 0xFFFFFFFF
    for what, s in (("an index >= G, last", raw(bad_last)), ("an index >= G, first", raw(bad_first)),
                    ("a range out of bounds", raw(g0=Gn - 4, n=5)), ("a range that wraps", raw(g0=1, n=0xFFFFFFFF)),
                    ("JG_GROUPS_DEVICE", raw(ok, flags=capi.GROUPS_DEVICE)), ("JG_GROUPS_DEVICE on a range", raw(n=5, flags=capi.GROUPS_DEVICE)),
                    ("n = JG_NODE_LOOKUP_MAX + 1", raw(np.zeros(MAX + 1, np.uint32))), ("a range of JG_NODE_LOOKUP_MAX + 1", raw(n=MAX + 1)),
                    ("self_slots", raw(ok, self_slots=ok.ctypes.data)), ("an unknown flag", raw(ok, flags=4)),
                    ("an unknown high flag", raw(ok, flags=capi.LOOKUP_PROGRESS | 1 << 31))):
        assert begin(s) == capi.EINVAL, what
    assert begin(raw(ok), flags & ~capi.NODE_KEEP) == capi.EINVAL  # a lookup travels with a kept step
    assert begin(raw(ok), flags & ~(capi.NODE_KEEP | capi.NODE_ASYNC)) == capi.EINVAL
    assert begin(raw(ok), flags & ~capi.NODE_ASYNC) == capi.EINVAL
    assert api.step_node_looked(None, 100, flags, None, None, C.byref(raw(ok))) == capi.EINVAL
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.step_node_begin(100, lookup=dict(groups=[1, 2]))
    with pytest.raises(EngineError):
        dev.step_node_begin(100, lookup=dict(groups=[0, Gn]), **kept)
    p = capi.Poll()
    p.want, p.g0, p.n = 32, 0, Gn  # a bad poll refuses the looked step too
    assert api.step_node_looked(h, 100, flags, C.byref(p), None, C.byref(raw(ok))) == capi.EINVAL
    same_step(dev.step_node(100), twin_step(100), "the plain step after the refusals")
    compare_snapshots(dev, twin, "the plain step after the refusals")
    with pytest.raises(EngineError):
        dev.node_lookup()  # (a plain step is no kept step)
    # n = JG_NODE_LOOKUP_MAX is accepted; the caller's list is free when the call returns
    submit(1)
    big = np.random.default_rng(2).integers(0, Gn, MAX).astype(np.uint32)
    lst = big.copy()
    assert begin(raw(lst, flags=capi.LOOKUP_PROGRESS)) == capi.OK
    lst[:] = 0xFFFFFFFF
    dev.__dict__.setdefault("_kept_backlog", []).append(False)  # (the mirror's note of the step begun behind its back)
    dev.__dict__.setdefault("_kept_await", []).append(None)
    first = twin_step(100) + (twin.lookup(big, progress=True),)
    # while it is outstanding the synchronous lookup stays refused
    with pytest.raises(EngineError, match="JG_NODE_KEEP"):
        dev.lookup()
    # a second step in flight: an empty lookup is attached, and has no rows
    submit(2)
    dev.step_node_begin(200, lookup=dict(groups=[], progress=True), **kept)
    second = twin_step(200)
    same_step(dev.node_outbox(), first, "the step of JG_NODE_LOOKUP_MAX entries")
    got = dev.node_lookup()
    lookup_equal(got, first[2], True, "the step of JG_NODE_LOOKUP_MAX entries")
    assert got["redone"] == (first[0]["rows_general"] > 0)
    lookup_equal(dev.node_lookup(), first[2], True, "the view may be asked again")
    same_step(dev.node_outbox(), second, "the step with an empty lookup")
    assert api.node_lookup_view(h, C.byref(v)) == capi.OK
    assert (v.attached, v.n) == (1, 0)
    got = dev.node_lookup()
    assert len(got["rows"]) == 0 and got["match"].shape == (0, R)
    # nothing is outstanding: the synchronous lookup works again
    same(dev.lookup(), twin.lookup(), "a lookup once the steps are viewed")
    # the rows of view t stay where they are, unchanged, after step t + 1 - with a lookup of its own - has begun
    submit(3)
    dev.step_node_begin(300, lookup=dict(g0=7, n=200, progress=True), **kept)
    third = twin_step(300) + (twin.lookup(g0=7, n=200, progress=True),)
    same_step(dev.node_outbox(), third, "the third step")
    assert api.node_lookup_view(h, C.byref(v)) == capi.OK
    assert (v.attached, v.n) == (1, 200) and v.rows and v.match
    at = lambda: (C.string_at(v.rows, 200 * 80), C.string_at(v.match, 200 * R * 8))  # noqa: E731
    held = at()
    assert held == (third[2][0].tobytes(), third[2][1].tobytes())
    submit(4)
    dev.step_node_begin(400, lookup=dict(groups=np.arange(250)[::-1], progress=True), **kept)
    fourth = twin_step(400) + (twin.lookup(np.arange(250)[::-1], progress=True),)
    assert at() == held
    w = capi.NodeLookup()
    assert api.node_lookup_view(h, C.byref(w)) == capi.OK and bytes(w) == bytes(v)  # (still the third step's)
    # a kept step without a lookup views attached == 0
    submit(5)
    dev.step_node_begin(500, **kept)
    plain = twin_step(500)
    same_step(dev.node_outbox(), fourth, "the fourth step")
    lookup_equal(dev.node_lookup(), fourth[2], True, "the fourth step")
    same_step(dev.node_outbox(), plain, "the kept step without a lookup")
    assert api.node_lookup_view(h, C.byref(v)) == capi.OK
    assert bytes(v) == bytes(C.sizeof(v))  # attached == 0 and everything else too
    assert dev.node_lookup() == {"redone": False}
    # lookup == NULL is exactly jg_step_node_awaited; all NULL is jg_step_node
    submit(6)
    assert api.step_node_looked(h, 600, flags & ~(capi.NODE_ASYNC | capi.NODE_KEEP), None, None, None) == capi.OK
    same_step(dev.node_outbox(), twin_step(600), "all NULL")
    compare_snapshots(dev, twin, "at the end")
    same(dev.lookup(), twin.lookup(), "at the end")
