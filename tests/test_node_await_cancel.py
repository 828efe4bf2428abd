"""A cancel behind a kept node step (ABI v24): jg_node_await_request.cancel_keys / cancel_n / cancel_mask and
jg_node_await.marked - withdrawing waiters with two ticks in flight.

The twin scheme of tests/test_node_await.py: a second device engine of the same seed and config is fed the same rows and
stepped synchronously, then asked await_blocks(rows), cancel_waiters(keys, mask) and watch_completions(...) with the step's
request.  What node_completions() hands out for kept step t - begun while step t - 1 was still outstanding - is that answer
byte for byte (rows, total, stats) and the twin's `marked`, on ticks whose chain came back redone and on plain ones; after the
last tick one peek over the whole table is equal on both.  Tokens are conn << 32 | seq.  On a third of the ticks a cancel
travels with the step: connections under the high mask or exact tokens, key counts on both sides of the 2 048 that fit the
mark pass's LDS, and always among them tokens the same step registers.  The cases with "small" in their ids also run on the
emulated device (tests/test_await_cancel_emulated.py)."""
import numpy as np
import pytest

from josefine_amd import capi
from node_step import compare_outboxes, node_traffic
from parity import compare_snapshots
from test_node_await import CAPACITY, G, HIGH, LOW, answer_equal, waiters
from test_node_poll import DRAINS, steady, twin_pair
from test_node_step import _same_rows

pytestmark = pytest.mark.gpu

T = 30
U = np.uint64
CONN_MASK = 0xFFFFFFFF00000000
CANCELLED = capi.DONE_CANCELLED
CONNS = 9


def cancel_of(kind, rng, registered, new_tokens):
    """the keys and the mask of cancel number `kind`: `registered` every token registered so far (many have left: decoys),
    `new_tokens` the ones this step registers"""
    mine = new_tokens[: max(1, len(new_tokens) // 4)]
    if kind % 4 == 0:  # one connection - a quarter of what this step registers goes with it or not, by its connection
        return np.array([int(mine[0]) >> 32 if len(mine) else 1], dtype=U) << U(32), CONN_MASK
    if kind % 4 == 2:  # three connections, one of them named twice
        c = rng.choice(np.arange(1, CONNS + 1), 3, replace=False).astype(U)
        return np.concatenate([c, c[:1]]) << U(32), CONN_MASK
    n = 2048 if kind % 4 == 1 else 3000  # exact tokens: the keys in LDS / in device memory
    old = rng.choice(registered, size=min(len(registered), 60), replace=False) if len(registered) else np.zeros(0, U)
    real = np.unique(np.concatenate([old, mine]).astype(U))
    decoys = (U(CONNS + 5) << U(32)) | np.arange(n - len(real), dtype=U)  # a connection nobody has
    keys = np.concatenate([real, decoys])
    assert len(np.unique(keys)) == n
    return keys[rng.permutation(n)], 2**64 - 1


@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="5")])
def test_awaited_steps_with_a_cancel_equal_the_twins_calls(R):
    dev, twin, rng = twin_pair(G, R, seed=31 + R)
    pick = np.random.default_rng(6)  # (the waiters' and the cancels' own stream)
    for e in (dev, twin):
        e.open_waiters(CAPACITY)

    def connected(w, token0):
        """the waiters' tokens as conn << 32 | seq"""
        n = len(w["groups"])
        w["tokens"] = (pick.integers(1, CONNS + 1, n).astype(U) << U(32)) | (np.arange(n, dtype=U) + U(token0))
        return w

    first = connected(waiters(pick, twin, 400, 0, 0, far=0.7), 1 << 20)
    for e in (dev, twin):
        assert e.await_blocks(**first) == 400
    registered = [first["tokens"]]
    want = []      # per tick: the twin's outbox, drains, answer, marked
    left = [400]   # the twin's table behind tick t - 1 (left[0]: before the first)
    begun = [0]    # rows registered by tick t - 1
    marks = {True: 0, False: 0}  # redone or not: waiters marked by the steps' cancels
    own = 0        # waiters a step's cancel withdrew that the same step registered
    kinds, states = 0, set()
    token, waiting = 0, 400

    def finish(t):
        b, drains, answer, marked = want[t]
        compare_outboxes(dev.node_outbox(), b, f"tick {t}")
        for fn in DRAINS:
            _same_rows(getattr(dev, fn)(), drains[fn], f"tick {t}: {fn}")
        got = dev.node_completions()
        answer_equal(got["answer"], answer, f"tick {t}")
        assert got["marked"] == marked, (t, got["marked"], marked)
        assert got["redone"] == (b["rows_general"] > 0), (t, got["redone"], b["rows_general"])
        marks[got["redone"]] += marked
        states.update(answer[0]["state"].tolist())

    for t in range(T):
        now = 100 * (t + 1)
        cols = node_traffic(rng, twin, token0=1000 * t, p_noise=0.03 if t % 3 else 0.0, p_reorder=0.08 if t % 3 else 0.0)
        if t % 3 == 0:  # every third tick is all steady state: its chain is the one queued behind the step, not redone
            cols = steady(cols, twin)
        # the library's bound: the table behind the newest VIEWED step (t - 2) and every row begun since (t - 1, t)
        bound = left[max(t - 1, 0)] + begun[t]
        room = min(CAPACITY - bound, HIGH - left[t])
        n = max(0, min(int(pick.integers(20, 70) + max(0, 500 - waiting)), room))
        new = connected(waiters(pick, twin, n, now, 0, far=0.8 if waiting < 500 else 0.1), token) if n else {}
        token += n
        w = dict(stats=True) if t % 2 else dict(limit=25, stats=True)
        request = dict(new, now_ms=now, **w)
        cancel = None
        if t % 6 in (0, 4):  # a third of the ticks, steady ones (0) and noisy ones (4) alike
            cancel = cancel_of(kinds, pick, np.concatenate(registered), new.get("tokens", np.zeros(0, U)))
            kinds += 1
            request.update(cancel_keys=cancel[0], cancel_mask=cancel[1])
        twin.submit_columns(**cols)
        b = twin.step_node(now)
        drains = {fn: getattr(twin, fn)() for fn in DRAINS}
        if n:
            assert twin.await_blocks(**new) == n
            assert LOW <= n + left[t] <= HIGH, (t, left)
            registered.append(new["tokens"])
        marked = 0
        if cancel is not None:
            marked = twin.cancel_waiters(*cancel)
            if n:
                own += int(np.isin(new["tokens"] & U(cancel[1]), cancel[0]).sum())
        answer = twin.watch_completions(now, w.get("limit"), False, stats=True)
        want.append((b, drains, answer, marked))
        begun.append(n)
        s = twin.watch_completions(now, limit=0, peek=True, stats=True)[2]
        left.append(s["left"])
        waiting = s["waiting"]
        dev.submit_columns(**cols)
        dev.step_node_begin(now, async_=True, keep=True, completions=request)
        if t % 9 == 4:  # a read between begin and view settles the newest step; the answer is what it would have been
            compare_snapshots(dev, twin, f"tick {t}, read while it is outstanding")
        if t:
            finish(t - 1)
    finish(T - 1)
    compare_snapshots(dev, twin, "after the last tick")
    assert kinds == 10 and marks[True] > 0 and marks[False] > 0 and own > 0, (kinds, marks, own)  # conditions of the test
    assert CANCELLED in states
    # nothing is outstanding: the synchronous calls again, on the one table - every waiter once, in registration order
    x, y = (e.watch_completions(100 * T, peek=True, stats=True) for e in (dev, twin))
    answer_equal(x, y, "a peek over the whole table afterwards")
    assert dev.cancel_waiters([0], 0) == twin.cancel_waiters([0], 0) == x[2]["left"] - x[2]["done"] + x[2]["applied"] + x[2]["lost"] + x[2]["expired"]
    x, y = (e.watch_completions(100 * T, stats=True) for e in (dev, twin))
    answer_equal(x, y, "everything withdrawn afterwards")
    assert x[2]["left"] == 0 and (x[0]["state"] == CANCELLED).all()
    for e in (dev, twin):
        e.open_waiters(0)


def test_small_rules():
    """a refused cancel refuses the step: nothing is stepped, the submitted rows stay queued"""
    import ctypes as C
    Gn, R = 300, 3
    dev, twin, rng = twin_pair(Gn, R, seed=5)
    api, h = dev.api, dev._h
    flags = capi.NODE_LEADER_HALF | capi.NODE_FOLLOWER_HALF | capi.NODE_TICK | capi.NODE_ASYNC | capi.NODE_KEEP
    for e in (dev, twin):
        e.open_waiters(10)
        assert e.await_blocks([1, 2, 3], 1 << 40, [11, 12, 13]) == 3
    cols = node_traffic(rng, twin, token0=0)
    twin.submit_columns(**cols), dev.submit_columns(**cols)
    keys = np.array([11, 13], dtype=U)
    many = np.arange(capi.AWAIT_CANCEL_MAX + 1, dtype=U)

    def raw(k, n, mask):
        q = capi.NodeAwaitRequest()
        q.cap, q.now_ms, q.want_stats = 8, 100, 1
        q.cancel_keys, q.cancel_n, q.cancel_mask = (k.ctypes.data if k is not None else None), n, mask
        return q

    for what, q in (("null keys", raw(None, 2, 2**64 - 1)), ("too many keys", raw(many, len(many), 2**64 - 1)),
                    ("a key with a bit outside the mask", raw(keys, 2, CONN_MASK))):
        assert api.step_node_awaited(h, 100, flags, None, C.byref(q)) == capi.EINVAL, what
    # the same step with a good cancel: the keys are copied at entry (the caller's array may go at once)
    k2 = keys.copy()
    q = raw(k2, 2, 2**64 - 1)
    assert api.step_node_awaited(h, 100, flags, None, C.byref(q)) == capi.OK
    k2[:] = 12
    # (the mirror's note of the step begun behind its back)
    dev.__dict__.setdefault("_kept_backlog", []).append(False), dev.__dict__.setdefault("_kept_await", []).append((True, True))
    b = twin.step_node(100)
    drains = {fn: getattr(twin, fn)() for fn in DRAINS}
    assert twin.cancel_waiters(keys) == 2
    answer = twin.watch_completions(100, limit=8, stats=True)
    compare_outboxes(dev.node_outbox(), b, "the step with a cancel")
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), drains[fn], f"the step with a cancel: {fn}")
    got = dev.node_completions()
    answer_equal(got["answer"], answer, "the step with a cancel")
    rows = got["answer"][0]
    assert got["marked"] == 2 and rows["state"][np.isin(rows["token"], [11, 13])].tolist() == [CANCELLED] * 2
    # a step without a cancel marks nothing
    dev.step_node_begin(200, async_=True, keep=True, completions=dict(now_ms=200, stats=True))
    twin.step_node(200)
    dev.node_outbox()
    assert dev.node_completions()["marked"] == 0
    for fn in DRAINS:
        _same_rows(getattr(dev, fn)(), getattr(twin, fn)(), f"the step without: {fn}")
    answer_equal(dev.watch_completions(200, peek=True, stats=True), twin.watch_completions(200, peek=True, stats=True), "afterwards")
    compare_snapshots(dev, twin, "at the end")
