"""jg_engine_await_cancel at 1 M slots, R = 5, every slot a leader, with 1 M waiters that wait (their blocks are far ahead),
tokens conn << 32 | seq over 100 connections: a cancel of ONE connection (1 % of the table) with one key, with 2 048 keys
(the most that are searched in LDS) and with 65 536 keys (searched in device memory) - the other keys are connections
nobody has - each call timed whole through the binding (best of three; the connection is registered again in between), and
the watch that follows it (it delivers the 1 % and compacts the table).  Beside them a plain device-to-device copy of the
table's 48 MB in the same run.  Run under rocprofv3 by profiles/micro/await_cancel_1m.sh; `--summarize DIR` turns that run's
kernel trace into the table of profiles/r16/await_cancel_1m.txt."""
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

WAITER_B = 48
CONNS = 100
HIGH = 0xFFFFFFFF00000000


def ms(t0):
    return round(1e3 * (time.perf_counter() - t0), 3)


def measure(reps=3):
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    from josefine_amd.traces import elect_all
    from vacant_groups_1m import copy_ms
    G, R, W = 1 << 20, 5, 1 << 20
    rng = np.random.default_rng(1)
    e = BatchedRaft(G, R, seed=1)
    elect_all(e, 10)
    e.drain_messages(), e.drain_applies(), e.drain_faults()
    e.open_waiters(W)
    conn = rng.integers(1, CONNS + 1, W).astype(np.uint64)
    groups = rng.integers(0, G, W)
    tokens = (conn << np.uint64(32)) | np.arange(W, dtype=np.uint64)
    e.await_blocks(groups, 1 << 40, tokens)
    r = dict(slots=G, R=R, waiters=W, connections=CONNS)
    victim = 1
    for n_keys in (1, 2048, 65536):
        cancel, watch, marked = [], [], []
        for _ in range(reps):
            mine = conn == victim
            keys = (np.concatenate([[victim], CONNS + 1 + np.arange(n_keys - 1)]).astype(np.uint64)) << np.uint64(32)
            keys = keys[rng.permutation(n_keys)]
            t0 = time.perf_counter()
            m = e.cancel_waiters(keys, HIGH)
            cancel.append(ms(t0))
            assert m == int(mine.sum()), (n_keys, m, int(mine.sum()))
            marked.append(m)
            t0 = time.perf_counter()
            rows, total = e.watch_completions(0)
            watch.append(ms(t0))
            assert total == m == len(rows) and (rows["state"] == capi.DONE_CANCELLED).all()
            e.await_blocks(groups[mine], 1 << 40, tokens[mine])  # the connection comes back: the table is 1 M again
            # (its waiters are at the table's end now: the victim's share is the same, the order is not)
            order = np.concatenate([np.nonzero(~mine)[0], np.nonzero(mine)[0]])
            conn, groups, tokens = conn[order], groups[order], tokens[order]
            victim = victim % CONNS + 1
        r[f"marked_{n_keys}"] = marked
        r[f"cancel_{n_keys}_keys_ms"], r[f"cancel_{n_keys}_keys_best_ms"] = cancel, min(cancel)
        r[f"watch_after_{n_keys}_keys_ms"], r[f"watch_after_{n_keys}_keys_best_ms"] = watch, min(watch)
    r["copy_table_bytes_ms"] = copy_ms(W * WAITER_B)
    print(json.dumps(r), flush=True)


def summarize(d):
    """the await kernels of a rocprofv3 run (its rocpd database), launch by launch"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    print(f"{'kernel':<40} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels where name like '%k_await%' group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        print(f"{name[:40]:<40} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f}")
    print("\nper-launch durations (us, in launch order: one repetition each of 1, 2 048 and 65 536 keys - the cancel, then the watch):")
    per = {}
    for name, x in c.execute("select name, duration from kernels where name like '%k_await%' order by start"):
        per.setdefault(name.split("(")[0].split(".")[0].strip(), []).append(round(x / 1e3, 1))
    for kn in ("k_await_mark", "k_await_mark_sum", "k_await_count", "k_await_write"):
        print(f"{kn:<20} {per.get(kn, [])}")
    print(f"\n(a waiter is {WAITER_B} B; the mark pass loads 16 B of it at a stride of 48: every 64-byte sector of the table, priced at {WAITER_B} B a waiter)")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    elif len(sys.argv) > 1 and sys.argv[1] == "--kernels-only":  # under a profiler: one repetition
        measure(reps=1)
    else:
        measure()
