"""jg_engine_poll at 1 M and 16 M slots, R = 5, every slot a leader: ONE poll of the three feeds against the three separate
calls (jg_engine_watch_leaders, jg_engine_watch_replicas, jg_engine_watch_commits) in sequence on a twin engine driven
identically, with 0 %, 1 % and 100 % of the partitions having moved since the last look, each timed whole on the host (best
of three).  The separate calls are the code as it was before ABI v18, measured in the same run.  Run under rocprofv3 by
profiles/micro/poll_1m.sh; `--summarize DIR` turns that run's kernel trace into the table of profiles/r12/poll_1m.txt: the
fused count pass per launch against the sum of the three count passes over the same slots."""
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

SEPARATE_B = (4 + 8 + 16 + 16) + (4 + 8 + 4) + (4 + 8 + 8 + 8 + 16)  # bytes per slot the three count passes read: 104
FUSED_B = SEPARATE_B - 4 - 4 - 8  # ... and the fused pass, the flag word and mlag read once: 88
COUNTS = ("k_watch_count", "k_isr_count", "k_commit_count")


def ms(t0):
    return round(1e3 * (time.perf_counter() - t0), 3)


def measure(sizes):
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    from josefine_amd.traces import elect_all
    lags = dict(leave_lag=4, join_lag=0)
    for G, R in sizes:
        es = [BatchedRaft(G, R, seed=1), BatchedRaft(G, R, seed=1)]  # [0]: the three calls; [1]: the poll
        for e in es:
            elect_all(e, 10)
            e.drain_messages(), e.drain_applies(), e.drain_faults()
        r = dict(slots=G, R=R)
        acks = np.full((R, G), capi.NO_ACK, np.uint64)

        def change(step):  # the leaders of every step-th slot append two blocks; all but one member acknowledge the head before them
            acks[:] = capi.NO_ACK
            acks[0, :] = 0  # (own slot: no appends)
            acks[0, ::step] = 2
            acks[1:, ::step] = es[0].read("head")[::step]
            acks[1, ::2 * step] = capi.NO_ACK  # (every other of them has a member that falls behind, then catches up)
            for e in es:
                e.step_dense_acks(acks)
                e.drain_messages(), e.drain_applies(), e.drain_faults()

        def calls(limit):
            a = es[0]
            return [a.watch_leaders(limit=limit)[1], a.watch_replicas(limit=limit, **lags)[1], a.watch_commits(limit=limit)[1]]

        def poll(limit):
            p = es[1].poll(leaders=dict(limit=limit), replicas=dict(lags, limit=limit), commits=dict(limit=limit))
            return [p[k][1] for k in ("leaders", "replicas", "commits")]

        change(1)
        t0 = time.perf_counter()
        first = calls(None)
        r["first_calls_ms"] = ms(t0)  # (allocate the shadows and the staging)
        t0 = time.perf_counter()
        assert poll(None) == first
        r["first_poll_ms"], r["first_totals"] = ms(t0), first
        for name, step, limit in (("one_percent", 100, G // 50), ("all", 1, None), ("quiet", None, G // 50)):
            c, p, tc, tp = [], [], [], []
            for _ in range(3):
                if step is not None:
                    change(step)
                t0 = time.perf_counter()
                tc.append(calls(limit))
                c.append(ms(t0))
                t0 = time.perf_counter()
                tp.append(poll(limit))
                p.append(ms(t0))
            assert tc == tp, (name, tc, tp)  # the twins see the same changes
            r[f"calls_{name}_ms"], r[f"poll_{name}_ms"], r[f"changed_{name}"] = c, p, tc
            r[f"calls_{name}_best_ms"], r[f"poll_{name}_best_ms"] = min(c), min(p)
        print(json.dumps(r), flush=True)
        del es


def summarize(d):
    """the kernels of a rocprofv3 run (its rocpd database), and the count passes launch by launch"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    print(f"{'kernel':<40} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        print(f"{name[:40]:<40} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f}")
    print("\nper-launch durations of the count passes (us, in launch order; per size one first look, then three looks each with")
    print("1 %, 100 % and nothing moved): the three separate passes, their sum, and the fused pass over the same slots")
    per = {}
    for kn in COUNTS + ("k_poll_count",):
        per[kn] = [round(x / 1e3, 1) for (x,) in c.execute("select duration from kernels where name like ? order by start", (f"%{kn}%",))]
        print(f"{kn:<16} {per[kn]}")
    n = min(len(v) for v in per.values())
    print(f"{'sum of three':<16} {[round(sum(per[k][i] for k in COUNTS), 1) for i in range(n)]}")
    print(f"{'k_poll_count':<16} {per['k_poll_count'][:n]}")
    print(f"\n(the three count passes read {SEPARATE_B} B per slot, the fused pass {FUSED_B} B: {FUSED_B << 20} B at 1 M slots, {FUSED_B << 24} B at 16 M)")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        pick = sys.argv[1] if len(sys.argv) > 1 else "all"
        sizes = [(G, 5) for G in (1 << 20, 1 << 24)]
        measure([s for s in sizes if pick == "all" or pick == f"{s[0]}x{s[1]}"])
