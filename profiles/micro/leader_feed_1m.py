"""jg_engine_watch_leaders / jg_engine_census at 1 M and 16 M slots (R = 3): a watch with 0 %, 1 % and 100 % of the slots
changed and a census, each call timed whole on the host (three repetitions), against (a) what a caller did before ABI v14 -
the six jg_read_state columns of the leadership view plus the numpy diff against the previous poll - and (b) a plain
device-to-device copy of the bytes the passes read (hipMemcpy, same device, same run).  Run under rocprofv3 by
profiles/micro/leader_feed_1m.sh; `--summarize DIR` turns that run's kernel trace into the table of
profiles/r09/leader_feed_1m.txt."""
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

R = 3
WATCH_B = 4 + 8 + 16 + 16  # bytes per slot one watch pass reads: flag word, term, cold_v record, shadow record
CENSUS_B = 4 + 8 + 16      # ... the census pass (a leader's mlag / head / commit on top)
COLS = ("role", "leader_id", "has_leader", "term", "fault", "self_slot")  # 16 bytes per slot


def ms(t0):
    return round(1e3 * (time.perf_counter() - t0), 3)


def measure():
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    from vacant_groups_1m import copy_ms
    out = []
    for G in (1 << 20, 1 << 24):
        e = BatchedRaft(G, R, seed=1)
        r = dict(slots=G, R=R)
        every = np.arange(G, dtype=np.uint32)
        some = every[::100].copy()
        now = [0]

        kind = {}

        def change(g):  # Timeout and Recreate in turn: follower at term 0 -> candidate at term 1 -> follower at term 0 ...
            k = kind[len(g)] = capi.CMD_RECREATE if kind.get(len(g)) == capi.CMD_TIMEOUT else capi.CMD_TIMEOUT
            e.submit_columns(np.full(len(g), k, np.uint8), g)
            now[0] += 10
            e.step(now[0])
            e.drain_messages(), e.drain_applies(), e.drain_faults()

        t0 = time.perf_counter()
        rows, total = e.watch_leaders()
        r["first_watch_ms"], r["first_watch_total"] = ms(t0), total  # (allocates the shadow and the staging)
        prev = [e.read(c) for c in COLS]

        def poll():  # (a): the six columns over the bus, then the diff on the host
            cur = [e.read(c) for c in COLS]
            m = cur[0] != prev[0]
            for a, b in zip(cur[1:], prev[1:]):
                m |= a != b
            prev[:] = cur
            return int(np.count_nonzero(m))

        for name, g, limit in (("one_percent", some, G // 50), ("all", every, None), ("quiet", None, G // 50)):
            w, p, tw, tp = [], [], [], []
            for _ in range(3):
                if g is not None:
                    change(g)
                t0 = time.perf_counter()
                rows, total = e.watch_leaders(limit=limit)
                w.append(ms(t0)), tw.append(total)
                t0 = time.perf_counter()
                tp.append(poll())
                p.append(ms(t0))
            assert tw == tp, (name, tw, tp)  # the feed and the poll see the same changes
            r[f"watch_{name}_ms"], r[f"poll_{name}_ms"], r[f"changed_{name}"] = w, p, tw
        t0 = time.perf_counter()
        total = e.watch_leaders(limit=0)[1]
        r["watch_quiet_count_only_ms"] = ms(t0)
        cs = []
        for _ in range(3):
            t0 = time.perf_counter()
            c = e.census()
            cs.append(ms(t0))
        r["census_ms"], r["census_followers"], r["census_candidates"] = cs, c["followers"], c["candidates"]
        r["copy_watch_pass_bytes_ms"] = copy_ms(G * WATCH_B)
        r["copy_census_pass_bytes_ms"] = copy_ms(G * CENSUS_B)
        out.append(r)
        del e
    for r in out:
        print(json.dumps(r))


def summarize(d):
    """the kernels of a rocprofv3 run (its rocpd database), and the feed's kernels launch by launch"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    print(f"{'kernel':<40} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        print(f"{name[:40]:<40} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f}")
    print("\nper-launch durations of the feed's kernels (us, in launch order; 1 M slots first, then 16 M):")
    for kn in ("k_watch_count", "k_watch_write", "k_census(", "k_census_sum"):
        ds = [round(x / 1e3, 1) for (x,) in c.execute("select duration from kernels where name like ? order by start", (f"%{kn}%",))]
        print(f"{kn:<20} {ds}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        measure()
