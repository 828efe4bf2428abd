"""jg_engine_watch_completions at 1 M slots, R = 5, every slot a leader, with W = 1 M and W = 4 M waiters registered in
shuffled (arrival) order, guarded by the leader's term: a tick after which 0 %, 1 % and 100 % of the waiters are done, the
registration and the watch each timed whole on the host (best of three), against (a) what a caller does today in the same
run - watch_commits rows, commit_rows_as_fsm, expand_fsm_rows and one dict probe per applied key (the dict filled with the
same waiters) - and (b) a plain device-to-device copy of the table's bytes (hipMemcpy, same device, same run).  Run under
rocprofv3 by profiles/micro/completion_feed_1m.sh; `--summarize DIR` turns that run's kernel trace into the table of
profiles/r14/completion_feed_1m.txt, `--pmc DIR` a counter run into bytes per waiter."""
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

WAITER_B = 48   # a waiter
GATHER_B = 44   # what the count pass uses of a slot: flag word, term, head, mlag, commit, run_hi
FAR = 10**12    # a deadline no timed watch reaches; the flush after it does


def ms(t0):
    return round(1e3 * (time.perf_counter() - t0), 3)


def measure(sizes, baseline=True, reps=3):
    import numpy as np
    from josefine_amd import BatchedRaft, capi, commit_rows_as_fsm, expand_fsm_rows
    from josefine_amd.traces import elect_all
    from vacant_groups_1m import copy_ms
    G, R = 1 << 20, 5
    rng = np.random.default_rng(1)
    e = BatchedRaft(G, R, seed=1)
    elect_all(e, 10)
    e.drain_messages(), e.drain_applies(), e.drain_faults()
    e.watch_commits()
    acks = np.full((R, G), capi.NO_ACK, np.uint64)

    def tick(sel, k):  # the leaders of `sel` append k blocks; a tick later everybody has acknowledged them
        for appends in (k, 0):
            acks[:] = capi.NO_ACK
            acks[0, :] = 0
            acks[0, sel] = appends
            acks[1:, :] = e.read("head")
            e.step_dense_acks(acks)
            e.drain_messages(), e.drain_applies(), e.drain_faults()

    for W in sizes:
        k = W // G
        e.open_waiters(W)
        wg = np.repeat(np.arange(G, dtype=np.int64), k)
        nth = np.tile(np.arange(k, dtype=np.int64), G)
        order = rng.permutation(W)
        wg, nth = wg[order], nth[order]  # arrival order: a partition's waiters are anywhere in the table
        tokens = np.arange(W, dtype=np.uint64)
        r = dict(slots=G, R=R, waiters=W, per_partition=k)
        for name, f in (("none", 0.0), ("one_percent", 0.01), ("all", 1.0)):
            reg, watch, fill, probe, totals, answered = [], [], [], [], [], []
            for _ in range(reps):
                sel = np.ones(G, bool) if f == 1.0 else rng.random(G) < f
                commit, term = e.read("commit").astype(np.int64), e.read("term").astype(np.uint64)
                ids = commit[wg] + 1 + nth + np.where(sel[wg], 0, 1000)  # the blocks the tick below appends, or far ones
                t0 = time.perf_counter()
                e.await_blocks(wg, ids, tokens, term[wg], FAR)
                reg.append(ms(t0))
                if baseline:
                    t0 = time.perf_counter()
                    d = dict(zip(((wg << 32) | ids).tolist(), tokens.tolist()))
                    fill.append(ms(t0))
                tick(sel, k)
                want = int(sel.sum()) * k
                t0 = time.perf_counter()
                rows, total = e.watch_completions(0, limit=None if f == 1.0 else W // 50)
                watch.append(ms(t0))
                assert total == want == len(rows) and (rows["state"] == capi.DONE_APPLIED).all(), (name, total, want, len(rows))
                totals.append(total)
                if baseline:
                    t0 = time.perf_counter()
                    crow, _ = e.watch_commits()
                    fsm = expand_fsm_rows(commit_rows_as_fsm(crow))
                    n = 0
                    for g, a, b in zip(fsm["group"].tolist(), fsm["a"].tolist(), fsm["b"].tolist()):  # (leaders: keys (a, b])
                        for key in range(a + 1, b + 1):
                            n += d.pop((g << 32) | key, None) is not None
                    probe.append(ms(t0))
                    answered.append(n)
                    del d
                else:
                    e.watch_commits()
                left = e.watch_completions(FAR + 1)  # the flush: the rest expires
                assert left[1] == W - want and e.watch_completions(limit=0, stats=True)[2]["left"] == 0
            if baseline:
                assert answered == totals, (name, answered, totals)
            r[f"done_{name}"] = totals
            r[f"register_{name}_ms"], r[f"watch_{name}_ms"] = reg, watch
            r[f"register_{name}_best_ms"], r[f"watch_{name}_best_ms"] = min(reg), min(watch)
            if baseline:
                r[f"dict_fill_{name}_ms"], r[f"dict_probe_{name}_ms"] = fill, probe
                r[f"dict_fill_{name}_best_ms"], r[f"dict_probe_{name}_best_ms"] = min(fill), min(probe)
        r["copy_table_bytes_ms"] = copy_ms(W * WAITER_B)
        r["copy_table_and_gather_bytes_ms"] = copy_ms(W * (WAITER_B + GATHER_B))
        print(json.dumps(r), flush=True)


def summarize(d):
    """the kernels of a rocprofv3 run (its rocpd database), and the feed's kernels launch by launch"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    print(f"{'kernel':<40} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        print(f"{name[:40]:<40} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f}")
    print("\nper-launch durations of the feed's kernels (us, in launch order; per table size W = 1 M then 4 M and per done fraction")
    print("0 %, 1 %, 100 %: one repetition = the timed watch, then the flush that expires what is left - nothing at 100 %):")
    for kn in ("k_await_count", "k_await_write", "k_await_stats_sum"):
        ds = [round(x / 1e3, 1) for (x,) in c.execute("select duration from kernels where name like ? order by start", (f"%{kn}%",))]
        print(f"{kn:<20} {ds}")
    print(f"\n(a waiter is {WAITER_B} B; the count pass uses {GATHER_B} B of its slot, from six 64-byte sectors)")


def pmc(d):
    """FETCH_SIZE / WRITE_SIZE (KiB) of the feed's kernels from a rocprofv3 --pmc run (csv), per launch"""
    rows = {}
    for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            kn = r.get("Kernel_Name", "")
            if "k_await" in kn:
                rows.setdefault((kn.split("(")[0], r.get("Counter_Name")), []).append(float(r.get("Counter_Value", 0)))
    if not rows:
        print("no counter rows found: not measured")
    for (kn, c), v in sorted(rows.items()):
        print(f"{kn:<20} {c:<12} KiB per launch: {[round(x) for x in v]}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "--pmc":
        pmc(sys.argv[2])
    elif len(sys.argv) > 1 and sys.argv[1] == "--kernels-only":  # under a profiler: no host baseline, one repetition
        measure([1 << 20, 1 << 22], baseline=False, reps=1)
    elif len(sys.argv) > 1 and sys.argv[1] == "--counters-only":
        measure([1 << 20], baseline=False, reps=1)
    else:
        measure([1 << 20, 1 << 22])
