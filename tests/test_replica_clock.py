"""Time-based in-sync sets (ABI v19): jg_engine_watch_replicas_timed, the replication feed under replica.lag.time.max.ms.
The view of a slot is a function of columns jg_read_state exposes (role, fault, self slot, head, match of every member, the
Replicate mask), of what the feed last delivered (`seen`) and of the feed's clocks (`stamp`: per member and slot, 0 or
now_ms + 1 of the first sample that saw the member behind), so the expected rows are stated in numpy over the engine's own
read(...) columns and the model's `seen` and `stamp` arrays - the rule of include/josefine_gpu.h written down once more,
independently of the kernel (which never forms c' for a member it can decide without it).  A timed watch returns exactly
the slots whose (isr, LEADS) differs from what the feed last delivered, ascending, every field equal; a call that does not
peek advances the clocks of its whole range, delivered or not; a peek advances nothing.  Cases whose id contains "small"
are small enough for the emulated device (tests/test_replica_clock_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, capi
from josefine_amd.engine import EngineError
from parity import compare_drains, compare_snapshots
from test_move_groups import drain_all
from test_replica_feed import BELOW, ISR_TILE, LEADS, SEEN_LEADS, U64_MAX, UNDER, dense_tick, elect, key_of, lags_of, popcount8, view_of

pytestmark = pytest.mark.gpu

NO = capi.NO_ACK
G_TILES = 2 * ISR_TILE + 37  # three workgroups of the watch passes, the last one ragged


def timed_view(e, seen, stamp, now, max_behind, caught, join, g0=0, n=None):
    """(the view of slots g0 .. g0 + n - 1 under the time rule as rows, the clocks [R][n] a call that does not peek leaves)"""
    n = e.G - g0 if n is None else n
    leads, head, lag, slot = lags_of(e, g0, n)
    sn = seen[g0:g0 + n]
    was = np.where(sn & SEEN_LEADS, sn & 0xff, 0)
    st = stamp[:, g0:g0 + n]
    now1 = np.uint64(now + 1)
    new = np.zeros_like(st)
    isr = np.zeros(n, np.uint8)
    for r in range(e.R):
        own = slot == r
        c = np.where(lag[r] <= np.uint64(caught), np.uint64(0), np.where(st[r] != 0, st[r], now1)).astype(np.uint64)
        behind_ms = np.where((c != 0) & (now1 > c), now1 - c, np.uint64(0)).astype(np.uint64)
        in_r = np.where((was >> r) & 1, behind_ms <= np.uint64(max_behind), lag[r] <= np.uint64(join))
        isr |= ((leads & (own | in_r)).astype(np.uint8) << r).astype(np.uint8)
        new[r] = np.where(leads, np.where(own, st[r], c), np.uint64(0))  # (the own slot's clock is ignored; not leading: 0)
    cnt = popcount8(isr)
    v = np.zeros(n, capi.ISR_ROW_DTYPE)
    v["group"], v["self_slot"], v["isr"] = g0 + np.arange(n), slot, isr
    v["replicate"] = np.where(leads, e.read("repl_state", 0, g0, n), 0)
    v["state"] = np.where(leads, LEADS | np.where(cnt < e.R, UNDER, 0) | np.where(cnt < e.R // 2 + 1, BELOW, 0), 0)
    v["head"] = np.where(leads, head, 0)
    v["worst_lag"] = np.where(leads, lag.max(axis=0), 0)
    return v, new


class Clock:
    """the test's statement of one engine's feed under the time rule: `seen` the (isr, LEADS) last delivered per slot, `stamp`
    the clocks"""

    def __init__(self, e, max_behind=500, caught=0, join=0):
        self.e, self.pol = e, dict(max_behind=max_behind, caught=caught, join=join)
        self.seen, self.stamp = np.zeros(e.G, np.uint16), np.zeros((e.R, e.G), np.uint64)

    def sample(self, now, what="", g0=0, n=None, limit=None, peek=False, other=None, **pol):
        """one timed watch against the model: the total, the rows, and the model moved on as the call moves the feed.
        `other`: an engine that is given the same call and has to answer the same.  Returns (rows, total)"""
        e = self.e
        p = dict(self.pol, **pol)
        n = e.G - g0 if n is None else n
        cur, new = timed_view(e, self.seen, self.stamp, now, p["max_behind"], p["caught"], p["join"], g0, n)
        m = key_of(cur) != self.seen[g0:g0 + n]
        want = cur[m] if limit is None else cur[m][:limit]
        rows, total = e.watch_replicas_timed(now, p["max_behind"], p["caught"], p["join"], g0, n, limit, peek)
        assert total == int(m.sum()), (what, now, total, int(m.sum()))
        assert rows.tobytes() == want.tobytes(), (what, now, rows[:4], want[:4])
        if other is not None:
            r2, t2 = other.watch_replicas_timed(now, p["max_behind"], p["caught"], p["join"], g0, n, limit, peek)
            assert t2 == total and r2.tobytes() == rows.tobytes(), (what, now, "the twin", t2, total)
        if not peek:
            self.stamp[:, g0:g0 + n] = new
            self.seen[rows["group"]] = key_of(rows)
        return rows, total

    def running(self, g):
        """the members of slot g whose clock runs, as a mask"""
        return sum(1 << r for r in range(self.e.R) if self.stamp[r, g])


def silent(G, on, ks):
    """an ack function for dense_tick: the members at the distances `ks` behind the own slot of the slots `on` say nothing"""
    on = np.isin(np.arange(G), on)
    return lambda k, head, slot: np.where(on & np.isin(k, ks), NO, head).astype(np.uint64)


everybody = lambda k, head, slot: head  # noqa: E731


def in_sync(both, appends=3):
    """appends that everybody acknowledges: lag 0 everywhere"""
    dense_tick(both, appends, everybody)
    dense_tick(both, 0, everybody)


def fall_behind(es, G, on, ks=(1,), appends=2):
    """appends that the members `ks` behind the own slot of the slots `on` do not acknowledge: they are `appends` blocks
    behind, everybody else has lag 0"""
    dense_tick(es, appends, silent(G, on, list(ks)))
    dense_tick(es, 0, silent(G, on, list(ks)))


def own_slots(G, R, layout):
    return np.full(G, R - 1, np.uint8) if layout == "uniform" else (np.arange(G) % R).astype(np.uint8)


# ---- 1. every transition, on one slot among quiet ones -----------------------------------------------------------------
@pytest.mark.parametrize("R,layout", [pytest.param(2, "uniform", id="small-2-uniform"), pytest.param(3, "mixed", id="small-3-mixed"),
                                      pytest.param(5, "uniform", id="small-5-uniform"), pytest.param(5, "mixed", id="small-5-mixed"),
                                      pytest.param(8, "mixed", id="small-8-mixed")])
def test_every_transition(R, layout):
    G = 96
    slots = own_slots(G, R, layout)
    e = BatchedRaft(G, R, seed=R, self_slots=slots)
    es = (e,)
    f = Clock(e, max_behind=500, caught=1, join=0)
    assert f.sample(900, "fresh")[1] == 0  # a fresh engine reports nothing until something leads
    gs = np.arange(0, G, 2)
    elect(es, gs, 10)
    rows, total = f.sample(1000, "elected")  # (a leader at genesis: every member's lag is 0, they join at once)
    assert total == len(gs) and (rows["isr"] == (1 << R) - 1).all() and (rows["state"] == LEADS).all()
    in_sync(es)
    assert f.sample(1001, "whole sets")[1] == 0
    X, self_x = int(gs[7]), int(slots[gs[7]])
    m1 = 1 << ((self_x + 1) % R)  # the member behind the own slot of X
    full = (1 << R) - 1
    # caught up -> behind starts the clock with no row; a lag of 1 <= caught_lag does not
    dense_tick(es, 1, silent(G, [X], [1]))
    assert f.sample(1100, "lag 1")[1] == 0 and f.running(X) == 0
    dense_tick(es, 1, silent(G, [X], [1]))
    dense_tick(es, 0, silent(G, [X], [1]))
    assert f.sample(1200, "behind")[1] == 0 and f.running(X) == m1 and not f.stamp[:, np.arange(G) != X].any()
    assert f.sample(1700, "inside the window, to its last millisecond")[1] == 0
    # caught up again before the window ends: the clock is cleared, and there is no row, ever
    dense_tick(es, 0, everybody)
    assert f.sample(1701, "caught up")[1] == 0 and f.running(X) == 0
    assert f.sample(9000, "later")[1] == 0
    # behind past the window: left
    dense_tick(es, 2, silent(G, [X], [1]))
    dense_tick(es, 0, silent(G, [X], [1]))
    assert f.sample(10000, "behind again")[1] == 0 and f.stamp[(self_x + 1) % R, X] == 10001
    assert f.sample(10500, "500 ms behind")[1] == 0
    rows, total = f.sample(10501, "501 ms behind")
    assert total == 1 and rows["group"][0] == X and rows["isr"][0] == full & ~m1 and (rows["state"][0] & UNDER)
    assert bool(rows["state"][0] & BELOW) == (R - 1 < R // 2 + 1) and rows["worst_lag"][0] == 2
    assert f.sample(20000, "it has left: nothing more")[1] == 0
    # everybody silent: the set shrinks to {self}, below quorum
    dense_tick(es, 2, silent(G, [X], list(range(1, R))))
    dense_tick(es, 0, silent(G, [X], list(range(1, R))))
    assert f.sample(30000, "all behind")[1] == 0
    rows, total = f.sample(30600, "all left")
    if R > 2:
        assert total == 1 and rows["isr"][0] == 1 << self_x and rows["state"][0] == LEADS | UNDER | BELOW
    else:
        assert total == 0
    # rejoin only at lag <= join_lag: an ack one block short is "caught up" for the clock and still outside
    dense_tick(es, 1, everybody)  # (the acks of a tick are those of the head before its appends: lag 1)
    assert f.sample(30700, "lag 1: not yet")[1] == 0 and f.running(X) == 0
    dense_tick(es, 0, everybody)
    rows, total = f.sample(30800, "rejoined")
    assert total == 1 and rows["isr"][0] == full and rows["state"][0] == LEADS
    # max_behind_ms = 0: in at the sample that sees it fall behind, and again at the same clock; out once the clock moves
    Z = int(gs[20])
    dense_tick(es, 2, silent(G, [Z], [1]))
    dense_tick(es, 0, silent(G, [Z], [1]))
    assert f.sample(40000, "0 ms: seen behind", max_behind=0)[1] == 0
    assert f.sample(40000, "0 ms: the same clock", max_behind=0)[1] == 0
    rows, total = f.sample(40001, "0 ms: the clock moved", max_behind=0)
    assert total == 1 and rows["group"][0] == Z and popcount8(rows["isr"])[0] == R - 1
    # max_behind_ms = UINT64_MAX: never leaves - and leaves at once under a finite window, for its clock ran all the time
    W = int(gs[30])
    fall_behind(es, G, [Z, W])  # (Z stays out: it would rejoin with its first ack)
    for now in (50000, 1 << 40, U64_MAX - 1):
        assert f.sample(now, "never", max_behind=U64_MAX)[1] == 0
    assert f.sample(U64_MAX - 1, "a window of 2^64 - 2 ms", max_behind=U64_MAX - 1)[1] == 0
    rows, total = f.sample(60000, "a finite window")
    assert total == 1 and rows["group"][0] == W
    # a new leader above genesis reports {self}: its members' progress starts over
    Y = int(gs[40])
    e.submit_columns(np.array([capi.CMD_RESTART], np.uint8), np.array([Y], np.uint32))
    e.step(70000)
    drain_all(e)
    rows, total = f.sample(70000, "restarted")
    assert total == 1 and rows["group"][0] == Y and rows["state"][0] == 0 and rows["isr"][0] == 0
    elect(es, [Y], 70100)
    rows, total = f.sample(70100, "a new leader")
    assert total == 1 and rows["group"][0] == Y and rows["isr"][0] == 1 << slots[Y] and rows["head"][0] > 0
    assert rows["state"][0] == LEADS | UNDER | BELOW
    assert not e.read("fault")[gs].any()


def test_small_one_member():
    """R = 1: the own slot alone - no clock is ever looked at"""
    G = 80
    e = BatchedRaft(G, 1, seed=1)
    f = Clock(e, max_behind=0)
    elect((e,), np.arange(0, G, 3), 10)
    rows, total = f.sample(5, "elected")
    assert total == len(range(0, G, 3)) and (rows["isr"] == 1).all() and (rows["state"] == LEADS).all()
    dense_tick((e,), 2, everybody)
    assert f.sample(10**6, "quiet")[1] == 0 and not f.stamp.any()


# ---- 2. cap and peek ---------------------------------------------------------------------------------------------------------
def whole_sets(G, R, seed=3):
    from josefine_amd.traces import elect_all
    e = BatchedRaft(G, R, seed=seed, self_slots=own_slots(G, R, "mixed"))
    elect_all(e, 10)
    drain_all(e)
    in_sync((e,))
    f = Clock(e, max_behind=500)
    assert f.sample(1000, "whole sets")[1] == G and (f.seen == (SEEN_LEADS | ((1 << R) - 1))).all()
    return e, f


def test_small_a_limit_still_advances_the_clocks_behind_it():
    G, R = G_TILES, 3
    e, f = whole_sets(G, R)
    down = np.arange(5, G, 7)
    shut = np.arange(0, 50)
    fall_behind((e,), G, down)
    e.close_groups(shut)
    # 50 rows are owed (the closed slots); 20 fit - and behind them the clocks start, in all three workgroups
    rows, total = f.sample(2000, "a limit that ends mid-range", limit=20)
    assert total == 50 and rows["group"].tolist() == list(range(20))
    led = down[down >= 50]
    assert (f.stamp[:, led] != 0).sum() == len(led) and led[-1] > 2 * ISR_TILE
    rows, total = f.sample(2500, "inside the window", limit=10)
    assert total == 30 and len(rows) == 10
    rows, total = f.sample(2501, "expired at the time the model says, and no later")
    assert total == 20 + len(led) and set(led.tolist()) <= set(rows["group"].tolist())
    assert f.sample(2501, "delivered")[1] == 0


def test_small_a_peek_changes_nothing():
    G, R = G_TILES, 3
    e, f = whole_sets(G, R)
    twin, ft = whole_sets(G, R)  # never peeked
    down = np.arange(3, G, 5)
    for x in (e, twin):
        fall_behind((x,), G, down)
    for now in (2000, 99999):  # members behind whose clocks do not run yet: a peek would start them
        assert f.sample(now, "peek before the clocks start", peek=True)[1] == 0
    for x in (f, ft):
        assert x.sample(2400, "the clocks start")[1] == 0
    rows, total = f.sample(99999, "a peek at a later time sees them leave", peek=True, limit=7)
    assert total == len(down) and rows["group"].tolist() == down[:7].tolist()
    assert f.sample(2000, "a peek at an earlier time", peek=True)[1] == 0
    for x in (f, ft):
        assert x.sample(2900, "500 ms after the start: still in")[1] == 0
    # two calls at one now_ms equal one
    for x in (f, ft):
        assert x.sample(2901, "left", limit=len(down) // 2)[1] == len(down)
    assert f.sample(2901, "the same clock again: the rest")[1] == len(down) - len(down) // 2
    assert ft.sample(2901, "the twin: the rest")[1] == len(down) - len(down) // 2
    assert np.array_equal(f.seen, ft.seen) and np.array_equal(f.stamp, ft.stamp)
    rows, total = e.watch_replicas_timed(2901, 500)
    assert total == 0 and twin.watch_replicas_timed(2901, 500)[1] == 0
    compare_snapshots(e, twin, "peeked and not")


# ---- 3. wide values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_wide_values(R):
    """clocks around 2^63 and up to UINT64_MAX - 1, a clock that steps back; heads above 2^32 with members whose lag fields
    are the BEHIND escape (a new leader's progress starts at 0) and the ABOVE escape (a forged ack above the head)"""
    G = 64
    hi = (1 << 32) + 5
    e = BatchedRaft(G, R, seed=2, self_slots=own_slots(G, R, "mixed"))
    e.load_chains([([(0, 0), (hi, 0)], hi)] * G, now_ms=10)
    elect((e,), np.arange(G), 20)
    assert (e.read("head") == hi).all()
    T0 = (1 << 63) - 3
    f = Clock(e, max_behind=10, caught=hi - 1, join=0)
    rows, total = f.sample(T0, "lag 2^32 + 5 against a join_lag of as much", caught=hi, join=hi)
    assert total == G and (rows["isr"] == (1 << R) - 1).all() and (rows["worst_lag"] == hi).all()
    assert f.sample(T0 + 1, "lag 2^32 + 5 against a caught_lag one short of it: the clocks start")[1] == 0
    assert (f.stamp != 0).sum() == G * (R - 1) and int(f.stamp.max()) == T0 + 2
    assert f.sample(T0 + 1, "caught up by a caught_lag that wide", caught=hi, join=0)[1] == 0 and not f.stamp.any()
    assert f.sample(T0 + 1, "... and behind again")[1] == 0
    assert f.sample(T0 + 5, "across 2^63, inside the window")[1] == 0 and T0 + 5 > 1 << 63
    assert f.sample(T0 - 100, "the clock steps back: nobody leaves")[1] == 0 and int(f.stamp.max()) == T0 + 2
    assert f.sample(0, "... all the way")[1] == 0
    # clocks that start at the last clock there is hold UINT64_MAX
    assert f.sample(T0 + 5, "cleared", caught=hi)[1] == 0 and not f.stamp.any()
    assert f.sample(U64_MAX - 1, "started at UINT64_MAX - 1")[1] == 0 and int(f.stamp.min()) == 0 and int(f.stamp.max()) == U64_MAX
    assert f.sample(U64_MAX - 1, "0 ms behind", max_behind=0)[1] == 0
    assert f.sample(T0, "back from there", max_behind=0)[1] == 0
    assert f.sample(T0 + 1, "cleared again", caught=hi)[1] == 0 and not f.stamp.any()
    assert f.sample(T0 + 1, "... and started again")[1] == 0 and int(f.stamp.max()) == T0 + 2
    # the member behind the own slot acknowledges the head; the next one of every other slot forges an ack above it
    forged = np.arange(G) % 2 == 0
    dense_tick((e,), 0, lambda k, head, slot: np.where(k == 1, head, np.where((k == 2) & forged, head + 50, NO)).astype(np.uint64))
    ok = forged & (e.read("fault") == 0)  # (the scenario exists: a forged ack stored above the head of a slot that goes on leading)
    m2 = np.array([e.read("match", int((g + 2) % R), int(g), 1)[0] for g in np.nonzero(ok)[0]])
    assert ok.any() and (m2 > hi).all()
    rows, total = f.sample(T0 + 12, "11 ms behind: those that said nothing leave")
    assert total >= G - int(forged.sum()) and ((rows["isr"] >> ((rows["self_slot"] + 1) % R)) & 1)[(rows["state"] & LEADS) != 0].all()
    assert f.sample(U64_MAX - 1, "the last clock there is")[1] == 0
    with pytest.raises(EngineError):
        e.watch_replicas_timed(U64_MAX, 10)


# ---- 4. a slot that does not lead clears its clocks --------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_not_leading_clears(R):
    G = 120
    slots = own_slots(G, R, "mixed")
    e = BatchedRaft(G, R, seed=5, self_slots=slots, election_timeout_ms=(300, 700))
    es = (e,)
    elect(es, np.arange(G), 10)
    in_sync(es)
    f = Clock(e, max_behind=500)
    assert f.sample(1000, "whole sets")[1] == G
    A = np.arange(0, 90)
    bad, shut, kept = A[:30], A[30:60], A[60:]  # faulted / closed with a sample in between; faulted with none
    fall_behind(es, G, A)
    assert f.sample(2000, "the clocks start")[1] == 0 and (f.stamp != 0).sum() == len(A)

    def fault(gs, now):  # an AppendResponse from a node the leader's progress does not know (progress.rs:43)
        gs = gs.astype(np.uint32)
        e.submit_columns(np.full(len(gs), capi.CMD_APPEND_RESPONSE, np.uint8), gs, from_=np.full(len(gs), 77, np.uint32),
                         term=e.read("term")[gs].astype(np.uint64), id=np.ones(len(gs), np.uint64), flag=np.ones(len(gs), np.uint8))
        e.step(now)
        drain_all(e)
        assert (e.read("fault")[gs] != 0).all()

    def again(gs, now):  # the process restarts on its tree and is elected again: its members' progress starts over
        e.submit_columns(np.full(len(gs), capi.CMD_RESTART, np.uint8), gs.astype(np.uint32))
        e.step(now)
        drain_all(e)
        elect(es, gs, now + 10)

    fault(bad, 2050)
    e.close_groups(shut)
    # one sample in between that delivers NOTHING: the shadow still holds the whole sets, the clocks are gone
    assert f.sample(2100, "not leading", limit=0)[1] == 60
    assert not f.stamp[:, :60].any() and (f.stamp[:, 60:90] != 0).sum() == 30
    again(bad, 2150)
    e.open_groups(shut, 2200)
    elect(es, shut, 2210)
    fault(kept, 2300)
    again(kept, 2310)  # ... and no sample in between: these keep their clocks, as they keep their shadow
    assert (e.read("role")[A] == capi.ROLE_LEADER).all() and (e.read("fault")[A] == 0).all()
    # a restarted leader's head is its commit index and its members' progress starts at 0: every member of `bad` and `kept`
    # is behind, and the shadow says it was in sync.  (An opened slot starts at genesis: lag 0, whole sets, as the shadow says)
    both = np.concatenate([bad, kept])
    assert (e.read("head")[both] > 0).all() and (e.read("head")[shut] == 0).all()
    rows, total = f.sample(2501, "fresh clocks for those that were seen not leading; 501 ms for those that were not")
    assert total == 30 and rows["group"].tolist() == kept.tolist() and (rows["isr"] == full_but(slots[kept], R, 1)).all()
    assert f.sample(3001, "500 ms after the fresh start")[1] == 0
    rows, total = f.sample(3002, "501 ms")
    assert total == 60 and rows["group"].tolist() == both.tolist() and (rows["isr"] == 1 << slots[both]).all()
    dense_tick(es, 0, everybody)
    assert not e.read("fault").any()
    assert f.sample(4000, "everybody back")[1] == 60 and (f.seen == (SEEN_LEADS | ((1 << R) - 1))).all() and not f.stamp.any()


def full_but(slot, R, k):
    """the whole set without the member k behind the own slot"""
    return (((1 << R) - 1) & ~(1 << ((slot.astype(np.int64) + k) % R))).astype(np.uint8)


# ---- 5. the lag rule and the time rule mixed on one engine ---------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_mixing(R):
    """One feed under two rules: lag watches and timed watches alternate on one engine against ONE model `seen` (the lag
    rule's rows are tests/test_replica_feed.py's view_of).  A twin is driven by the timed calls alone.  The clocks do not
    depend on the shadow, so the two models' clocks are equal throughout; and a lag watch that is followed by a timed watch
    on unchanged state, under a lag policy nobody leaves by (leave_lag = UINT64_MAX, join_lag = the timed join_lag), only
    delivers EARLIER what the timed watch would have: then every timed row of the mixed engine is the twin's row of that slot,
    and the twin's other rows are those the lag watch took.  Afterwards the two feeds have seen the same."""
    G = 150
    rng = np.random.default_rng(R)
    slots = own_slots(G, R, "mixed")
    a, b = (BatchedRaft(G, R, seed=7, self_slots=slots) for _ in range(2))
    both = (a, b)
    lead = np.arange(G) % 3 != 2
    elect(both, np.nonzero(lead)[0], 10)
    fa, fb = Clock(a, max_behind=250, caught=1, join=0), Clock(b, max_behind=250, caught=1, join=0)

    def lag_watch(leave, join, **kw):
        cur = view_of(a, fa.seen, leave, join)
        m = key_of(cur) != fa.seen
        rows, total = a.watch_replicas(leave, join, **kw)
        want = cur[m][:kw.get("limit")]
        assert total == int(m.sum()) and rows.tobytes() == want.tobytes(), (leave, join, total, int(m.sum()))
        if not kw.get("peek"):
            fa.seen[rows["group"]] = key_of(rows)
        return rows

    now, agreed, early = 1000, 0, 0
    for t in range(24):
        quiet = rng.random((R, G)) < 0.25
        dense_tick(both, int(rng.integers(0, 3)), lambda k, head, slot: np.where(quiet[k], NO, head).astype(np.uint64))
        if t in (6, 18):
            for x in both:
                x.close_groups(np.arange(t, t + 10))
        now += int(rng.integers(0, 200))
        if t < 12:  # the lag watch straight before the timed one
            assert np.array_equal(fa.seen, fb.seen), t
            took = lag_watch(U64_MAX, 0)
            rb, _ = fb.sample(now, f"twin {t}")
            ra, _ = fa.sample(now, f"mixed {t}")
            agreed += 1
            early += len(took)
            by_group = {int(r["group"]): r.tobytes() for r in rb}
            assert all(by_group.get(int(r["group"])) == r.tobytes() for r in ra), t
            rest = set(by_group) - set(ra["group"].tolist())
            assert rest <= set(took["group"].tolist()), (t, sorted(rest)[:5])
            assert np.array_equal(fa.seen, fb.seen), t
        else:  # a lag policy of its own, a tick between the two watches: against the model alone
            lag_watch(3, 1, limit=int(rng.integers(0, 40)), peek=bool(t % 4 == 1))
            dense_tick(both, 1, lambda k, head, slot: np.where(quiet[k], NO, head).astype(np.uint64))
            fb.sample(now, f"twin {t}")
            fa.sample(now, f"mixed {t}", limit=int(rng.integers(0, 60)))
        assert np.array_equal(fa.stamp, fb.stamp), t
    assert agreed == 12 and early > 0 and (fa.stamp != 0).any()
    compare_snapshots(a, b, "mixed and timed only")


# ---- 6. shards -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [pytest.param(2, id="small-2-shards"), pytest.param(3, id="small-3-shards")])
def test_shards(D):
    G, R = 1000, 3
    s = BatchedRaft(G, R, seed=4, device_ids=[0] * D)
    one = BatchedRaft(G, R, seed=4)
    both = (s, one)
    last, first = s.shard(D - 1).group_lo, s.shard(0).G
    f = Clock(s, max_behind=500)
    assert f.sample(5, "fresh", other=one)[1] == 0
    for e in both:
        elect((e,), np.arange(G), 10)
        in_sync((e,))
    f.sample(1000, "count", limit=0, other=one)
    f.sample(1000, "a range across the shard border", g0=first - 5, n=11, peek=True, other=one)
    rows, total = f.sample(1000, "a range across the shard border, delivered", g0=first - 5, n=11, other=one)
    assert total == 11
    assert f.sample(1000, "the rest", other=one)[1] == G - 11
    down = np.concatenate([np.arange(3, first, 50), np.arange(last + 1, G, 9)])
    shut = np.arange(0, 40)
    for e in both:
        fall_behind((e,), G, down)
        e.close_groups(shut)
    # a limit that ends inside the first shard ...
    rows, total = f.sample(2000, "a limit that ends inside the first shard", limit=15, other=one)
    assert total == 40 and rows["group"].tolist() == list(range(15)) and 15 < first
    assert (f.stamp[:, last:] != 0).sum() == int((down >= last).sum()) > 5
    assert f.sample(2500, "inside the window", limit=5, other=one)[1] == 25
    # ... followed by expiry in the last shard, at the time the model says
    rows, total = f.sample(2501, "expiry", other=one)
    led = down[down >= 40]
    assert total == 20 + len(led) and set(led.tolist()) <= set(rows["group"].tolist()) and rows["group"][-1] >= last
    assert f.sample(2501, "quiet", other=one)[1] == 0
    f.sample(9000, "the last shard alone, peeked", g0=last, n=G - last, limit=3, peek=True, other=one)
    for e in both:
        in_sync((e,))
    assert f.sample(9000, "back", other=one)[1] == len(led)
    compare_snapshots(s, one, "shards")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_small_refusals():
    G, R = 200, 3
    e, twin = BatchedRaft(G, R, seed=4), BatchedRaft(G, R, seed=4)
    for x in (e, twin):
        elect((x,), np.arange(50), 10)
    api, h = e.api, e._h
    rows = np.zeros(G, capi.ISR_ROW_DTYPE)
    total = C.c_size_t(0)
    clk = capi.IsrClock(1000, 500, 4, 1)
    watch = lambda flags, c, g0, n, out, cap, tot: api.engine_watch_replicas_timed(h, flags, c, g0, n, out, cap, tot)  # noqa: E731
    K = C.byref(clk)

    def pending():  # nothing was advanced: a peek shows the 50 new leaders still
        t = C.c_size_t(0)
        assert watch(capi.WATCH_PEEK, K, 0, G, None, 0, C.byref(t)) == capi.OK
        return t.value

    assert pending() == 50
    refused = [
        lambda: watch(0, K, 0, G, rows.ctypes.data, G, None),                     # a null total
        lambda: watch(0, K, 0, G, None, 5, C.byref(total)),                       # a null out with cap > 0
        lambda: watch(2, K, 0, G, rows.ctypes.data, G, C.byref(total)),           # an unknown flag
        lambda: watch(0, K, G - 1, 2, rows.ctypes.data, G, C.byref(total)),       # a range out of bounds
        lambda: watch(0, K, 1, 0xFFFFFFFF, rows.ctypes.data, G, C.byref(total)),  # ... that wraps in 32 bits
        lambda: watch(0, None, 0, G, rows.ctypes.data, G, C.byref(total)),        # a null clock
        lambda: watch(0, C.byref(capi.IsrClock(U64_MAX, 500, 4, 1)), 0, G, rows.ctypes.data, G, C.byref(total)),  # now_ms
        lambda: watch(0, C.byref(capi.IsrClock(1000, 500, 1, 4)), 0, G, rows.ctypes.data, G, C.byref(total)),    # join > caught
        lambda: api.engine_watch_replicas_timed(None, 0, K, 0, G, rows.ctypes.data, G, C.byref(total)),           # a null engine
    ]
    total.value = 77
    for k, call in enumerate(refused):
        assert call() == capi.EINVAL, k
        assert total.value == 77 and not rows.view(np.uint8).any(), k  # nothing written
        assert pending() == 50, k
    with pytest.raises(EngineError):
        e.watch_replicas_timed(1000, 500, 1, 4)
    assert watch(0, K, 7, 0, None, 0, C.byref(total)) == capi.OK and total.value == 0  # n = 0
    # kept node steps outstanding: refused with read_chains's code, and the kept steps are still viewable afterwards
    for x in (e, twin):
        x.step_node_begin(1000, async_=True, keep=True)
        x.step_node_begin(1100, async_=True, keep=True)
    r = capi.ChainRead()
    r.n, off = G, np.zeros(G + 1, np.uint64)
    r.off = off.ctypes.data
    code = api.engine_read_chains(h, C.byref(r), C.byref(C.c_uint64(0)))
    assert code == capi.EINVAL
    total.value = 77
    assert watch(0, K, 0, G, rows.ctypes.data, G, C.byref(total)) == code and total.value == 77
    assert watch(capi.WATCH_PEEK, K, 0, G, rows.ctypes.data, G, C.byref(total)) == code and not rows.view(np.uint8).any()
    with pytest.raises(EngineError):
        e.watch_replicas_timed(1000, 500)
    outs = [[x.node_outbox(), x.node_outbox()] for x in (e, twin)]
    for k in range(2):
        for name, v in outs[0][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][k][name])), (k, name)
    compare_drains(e, twin, "kept")
    compare_snapshots(e, twin, "kept")
    # the twin was never watched: the calls change nothing a step or a drain observes
    f = Clock(e, max_behind=500, caught=1, join=1)
    assert f.sample(1000, "after the refusals")[1] == 50
    for t in range(3):
        for x in (e, twin):
            fall_behind((x,), G, np.arange(0, 50, 2))
        f.sample(2000 + 400 * t, f"tick {t}")
        compare_drains(e, twin, f"tick {t}")
        compare_snapshots(e, twin, f"tick {t}")
    assert (popcount8(f.seen[:50:2] & 0xff) == R - 1).all()


# ---- 8. a seeded walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [pytest.param(3, id="small-3"), pytest.param(5, id="small-5")])
def test_seeded_walk(R):
    G = 100
    rng = np.random.default_rng(100 + R)
    e = BatchedRaft(G, R, seed=9, self_slots=rng.integers(0, R, G).astype(np.uint8))
    led = np.nonzero(rng.random(G) < 0.8)[0]
    elect((e,), led, 10)
    f = Clock(e, max_behind=300, caught=2, join=1)
    now, delivered, left, back = 1000, 0, 0, 0
    quiet = rng.random((R, G)) < 0.3
    for t in range(200):
        if t % 10 == 0:  # who is silent changes every ten samples: long enough to leave, and to come back
            quiet = rng.random((R, G)) < 0.3
        dense_tick((e,), int(rng.integers(0, 4)), lambda k, head, slot: np.where(quiet[k], NO, head).astype(np.uint64))
        now += int(rng.choice([0, 0, 1, 50, 150, 400]))
        before = f.seen.copy()
        kw = {}
        if rng.random() < 0.3:
            kw["limit"] = int(rng.integers(0, 30))
        if rng.random() < 0.15:
            kw["peek"] = True
        if rng.random() < 0.2:
            kw["g0"] = int(rng.integers(0, G))
            kw["n"] = int(rng.integers(1, G - kw["g0"] + 1))
        rows, _ = f.sample(now, f"sample {t}", **kw)
        delivered += len(rows)
        both_lead = ((before & SEEN_LEADS) != 0) & ((f.seen & SEEN_LEADS) != 0)
        left += int((both_lead & ((before & ~f.seen & 0xff) != 0)).sum())
        back += int((both_lead & ((f.seen & ~before & 0xff) != 0)).sum())
    assert left > 20 and back > 20 and delivered > 100, (left, back, delivered)
    assert not e.read("fault")[led].any()
