"""jg_engine_watch_replicas_timed at 1 M slots, R = 5, every slot a leader, beside jg_engine_watch_replicas on the SAME engine
in the same run (the lag feed's code is unchanged by ABI v19): three samples, each call timed whole on the host (best of
three) -
  quiet    every follower caught up, no clock running: the timed count pass reads 17 bytes per slot (flag word, mlag, shadow
           word, mask byte), the lag feed's 16
  running  1 % of the followers silent, their clocks running inside the window (the sample that starts the clocks is timed
           once, before): the stamp of every such member is read
  expiry   the sample where they expire: a row per slot with such a member.  Timed as peeks (three each; the lag feed beside
           it under a leave_lag those members are past, so it owes the same slots), then once for real
Run under rocprofv3 by profiles/micro/isr_clock_1m.sh; `--summarize DIR` turns that run's kernel trace into the table of
profiles/r13/isr_clock_1m.txt: the count passes of the two feeds launch by launch."""
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

LAG_B, TIMED_B = 4 + 8 + 4, 4 + 8 + 4 + 1  # bytes per slot the two count passes read while nothing runs
WINDOW = 30_000


def ms(t0):
    return round(1e3 * (time.perf_counter() - t0), 3)


def measure(G, R):
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    from josefine_amd.traces import elect_all
    e = BatchedRaft(G, R, seed=1)
    elect_all(e, 10)
    drain = lambda: (e.drain_messages(), e.drain_applies(), e.drain_faults())  # noqa: E731
    drain()
    rng = np.random.default_rng(6)
    down = rng.random((R, G)) < 0.01  # (member slot, slot): about 1 % of the followers
    down[0, :] = False                # (slot 0 is every leader's own)
    acks = np.full((R, G), capi.NO_ACK, np.uint64)

    def tick(appends, silent):
        acks[:] = e.read("head")
        acks[0, :] = appends
        if silent:
            acks[down] = capi.NO_ACK
        e.step_dense_acks(acks)
        drain()

    tick(3, False)
    tick(0, False)
    limit = G // 10
    r = dict(slots=G, R=R, limit=limit, window_ms=WINDOW, silent_members=int(down.sum()), slots_with_one=int(down.any(axis=0).sum()))
    t0 = time.perf_counter()
    first = e.watch_replicas_timed(1000, WINDOW)[1]
    r["first_timed_ms"], r["first_total"] = ms(t0), first  # (allocates the shadow, the clocks and the staging; delivers every slot)
    assert first == G and e.watch_replicas(1 << 40, 0)[1] == 0

    def best(name, timed, lag, want_timed, want_lag, n=3):
        a, b = [], []
        for _ in range(n):
            t0 = time.perf_counter()
            tt = timed()[1]
            a.append(ms(t0))
            t0 = time.perf_counter()
            tl = lag()[1]
            b.append(ms(t0))
            assert (tt, tl) == (want_timed, want_lag), (name, tt, tl, want_timed, want_lag)
        r[f"{name}_timed_ms"], r[f"{name}_lag_ms"] = a, b
        r[f"{name}_timed_best_ms"], r[f"{name}_lag_best_ms"], r[f"{name}_totals"] = min(a), min(b), [want_timed, want_lag]

    now = [2000]

    def timed(peek=False, at=None):
        now[0] += 100
        return e.watch_replicas_timed(now[0] if at is None else at, WINDOW, limit=limit, peek=peek)

    best("quiet", timed, lambda: e.watch_replicas(1 << 40, 0, limit=limit), 0, 0)
    tick(2, True)
    tick(0, True)
    started = now[0] + 100
    t0 = time.perf_counter()
    assert timed()[1] == 0
    r["start_timed_ms"] = ms(t0)  # (the sample that starts the clocks: a stamp and a mask byte stored per silent member)
    best("running", timed, lambda: e.watch_replicas(1 << 40, 0, limit=limit), 0, 0)
    owed = r["slots_with_one"]
    late = started + WINDOW + 1
    best("expiry_peek", lambda: timed(True, late), lambda: e.watch_replicas(1, 0, limit=limit, peek=True), owed, owed)
    t0 = time.perf_counter()
    rows, total = timed(False, late)
    r["expiry_timed_ms"], r["expiry_rows"] = ms(t0), len(rows)
    assert total == owed and len(rows) == min(owed, limit)
    print(json.dumps(r), flush=True)


def summarize(d):
    """the kernels of a rocprofv3 run (its rocpd database), and the count passes of the two feeds launch by launch"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    print(f"{'kernel':<40} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels where name like '%k_isr%' or name like '%k_scan_block%' group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        print(f"{name[:40]:<40} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f}")
    print("\nper-launch durations (us, in launch order).  k_isrc_count: the first look, 3 quiet, the start, 3 running, 3 expiry")
    print("peeks, the expiry.  k_isr_count: one look after the first, then 3 quiet, 3 running (quiet for the lag rule), 3 expiry peeks")
    for kn in ("k_isrc_count", "k_isr_count", "k_isrc_write", "k_isr_write"):
        per = [round(x / 1e3, 1) for (x,) in c.execute("select duration from kernels where name like ? order by start", (f"%{kn}%",))]
        print(f"{kn:<14} {per}")
    print(f"\n(quiet, the timed count pass reads {TIMED_B} B per slot, the lag feed's {LAG_B} B: {TIMED_B << 20} B against {LAG_B << 20} B at 1 M slots)")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        measure(1 << 20, 5)
