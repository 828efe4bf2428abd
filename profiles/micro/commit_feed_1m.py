"""jg_engine_watch_commits at 1 M and 16 M slots, R = 5, every slot a leader: a watch with 0 %, 1 % and 100 % of the
partitions having moved since the last poll and the count alone (`cap` 0, with the backlog), each call timed whole on the
host (best of three), against (a) what a caller did before ABI v17 - read("commit") + read("head") over the whole range and
a numpy diff against a host copy - and (b) a plain device-to-device copy of the bytes the count pass reads (hipMemcpy, same
device, same run).  Run under rocprofv3 by profiles/micro/commit_feed_1m.sh; `--summarize DIR` turns that run's kernel trace
into the table of profiles/r11/commit_feed_1m.txt."""
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

COUNT_B = 4 + 8 + 8 + 8 + 16  # bytes per slot the count pass reads: flag word, head, mlag, the commit column, the shadow


def ms(t0):
    return round(1e3 * (time.perf_counter() - t0), 3)


def measure(sizes):
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    from josefine_amd.traces import elect_all
    from vacant_groups_1m import copy_ms
    for G, R in sizes:
        e = BatchedRaft(G, R, seed=1)
        elect_all(e, 10)
        e.drain_messages(), e.drain_applies(), e.drain_faults()
        r = dict(slots=G, R=R)
        acks = np.full((R, G), capi.NO_ACK, np.uint64)

        def change(step):  # the leaders of every step-th slot append two blocks; everybody acknowledges the head before them
            acks[:] = capi.NO_ACK
            acks[0, :] = 0  # (own slot: no appends)
            acks[0, ::step] = 2
            acks[1:, ::step] = e.read("head")[::step]
            e.step_dense_acks(acks)
            e.drain_messages(), e.drain_applies(), e.drain_faults()

        change(1)
        t0 = time.perf_counter()
        rows, total = e.watch_commits()
        r["first_watch_ms"], r["first_watch_total"] = ms(t0), total  # (allocates the shadow and the staging)
        prev = [np.stack([e.read("commit"), e.read("head")])]

        def poll():  # (a): the two columns over the bus, the diff on the host
            cur = np.stack([e.read("commit"), e.read("head")])
            n = int(np.count_nonzero((cur != prev[0]).any(axis=0)))
            prev[0] = cur
            return n

        for name, step, limit in (("one_percent", 100, G // 50), ("all", 1, None), ("quiet", None, G // 50)):
            w, p, tw, tp = [], [], [], []
            for _ in range(3):
                if step is not None:
                    change(step)
                t0 = time.perf_counter()
                rows, total = e.watch_commits(limit=limit)
                w.append(ms(t0)), tw.append(total)
                t0 = time.perf_counter()
                tp.append(poll())
                p.append(ms(t0))
            assert tw == tp, (name, tw, tp)  # the feed and the poll see the same changes
            r[f"watch_{name}_ms"], r[f"poll_{name}_ms"], r[f"changed_{name}"] = w, p, tw
            r[f"watch_{name}_best_ms"], r[f"poll_{name}_best_ms"] = min(w), min(p)
        cs = []
        for _ in range(3):
            t0 = time.perf_counter()
            e.watch_commits(limit=0, backlog=True)
            cs.append(ms(t0))
        r["watch_quiet_count_and_backlog_ms"] = cs
        r["copy_count_pass_bytes_ms"] = copy_ms(G * COUNT_B)
        print(json.dumps(r), flush=True)
        del e


def summarize(d):
    """the kernels of a rocprofv3 run (its rocpd database), and the feed's kernels launch by launch"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    print(f"{'kernel':<40} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        print(f"{name[:40]:<40} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f}")
    print("\nper-launch durations of the feed's kernels (us, in launch order; the sizes in the order of the run: per size one first")
    print("watch, then three watches each with 1 %, 100 % and nothing moved, then three counts with the backlog):")
    for kn in ("k_commit_count", "k_commit_write", "k_commit_backlog_sum"):
        ds = [round(x / 1e3, 1) for (x,) in c.execute("select duration from kernels where name like ? order by start", (f"%{kn}%",))]
        print(f"{kn:<22} {ds}")
    print(f"\n(the count pass reads {COUNT_B} B per slot: {COUNT_B << 20} B at 1 M slots, {COUNT_B << 24} B at 16 M)")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        pick = sys.argv[1] if len(sys.argv) > 1 else "all"
        sizes = [(G, 5) for G in (1 << 20, 1 << 24)]
        measure([s for s in sizes if pick == "all" or pick == f"{s[0]}x{s[1]}"])
