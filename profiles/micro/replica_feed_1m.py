"""jg_engine_watch_replicas / jg_engine_replication_census at 1 M and 16 M slots, R = 3 and R = 5, every slot a leader: a
watch with 0 %, 1 % and 100 % of the in-sync sets changed, the count alone (`cap` 0) and a census, each call timed whole on
the host (three repetitions), against (a) what a caller did before ABI v15 - the jg_read_state columns of the replication
view (role, fault, self slot, head and MATCH of every member: 8R + 14 bytes per slot) plus the numpy threshold and diff
against the previous poll - and (b) a plain device-to-device copy of the bytes the count pass reads (hipMemcpy, same device,
same run).  Run under rocprofv3 by profiles/micro/replica_feed_1m.sh; `--summarize DIR` turns that run's kernel trace into
the table of profiles/r10/replica_feed_1m.txt."""
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

COUNT_B = 4 + 8 + 4  # bytes per slot the count pass reads: flag word, packed progress word, shadow word
CENSUS_B = 4 + 8     # ... the census pass
LAG = 4              # leave_lag == join_lag == lag_limit of the run


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
        t0 = time.perf_counter()
        rows, total = e.watch_replicas(LAG)
        r["first_watch_ms"], r["first_watch_total"] = ms(t0), total  # (allocates the shadow and the staging)
        acks = np.full((R, G), capi.NO_ACK, np.uint64)
        out_now = {}

        def change(step):  # the leaders of every step-th slot append LAG + 2 blocks nobody acknowledges / are acknowledged
            acks[:] = capi.NO_ACK
            acks[0, :] = 0  # (own slot: no appends)
            if out_now.get(step):
                acks[1:, ::step] = e.read("head")[::step]
                acks[0, ::step] = 0
            else:
                acks[0, ::step] = LAG + 2
            out_now[step] = not out_now.get(step)
            e.step_dense_acks(acks)
            e.drain_messages(), e.drain_applies(), e.drain_faults()

        def view():  # (a): the columns over the bus, the threshold on the host
            role, fault, slot, head = e.read("role"), e.read("fault"), e.read("self_slot"), e.read("head")
            leads = (role == capi.ROLE_LEADER) & (fault == 0)
            isr = np.zeros(G, np.uint16)
            for k in range(R):
                m = e.read("match", k)
                isr |= (leads & ((slot == k) | (head <= m) | (head - m <= LAG))).astype(np.uint16) << k
            return isr | (leads.astype(np.uint16) << 8)

        prev = [view()]

        def poll():
            cur = view()
            n = int(np.count_nonzero(cur != prev[0]))
            prev[0] = cur
            return n

        for name, step, limit in (("one_percent", 100, G // 50), ("all", 1, None), ("quiet", None, G // 50)):
            w, p, tw, tp = [], [], [], []
            for _ in range(3):
                if step is not None:
                    change(step)
                t0 = time.perf_counter()
                rows, total = e.watch_replicas(LAG, limit=limit)
                w.append(ms(t0)), tw.append(total)
                t0 = time.perf_counter()
                tp.append(poll())
                p.append(ms(t0))
            assert tw == tp, (name, tw, tp)  # the feed and the poll see the same changes
            r[f"watch_{name}_ms"], r[f"poll_{name}_ms"], r[f"changed_{name}"] = w, p, tw
        t0 = time.perf_counter()
        e.watch_replicas(LAG, limit=0)
        r["watch_quiet_count_only_ms"] = ms(t0)
        change(100)  # (a census of something: 1 % of the slots under-replicated)
        cs = []
        for _ in range(3):
            t0 = time.perf_counter()
            c = e.replication_census(LAG)
            cs.append(ms(t0))
        r["census_ms"], r["census_leaders"], r["census_under_replicated"] = cs, c["leaders"], c["under_replicated"]
        r["copy_count_pass_bytes_ms"] = copy_ms(G * COUNT_B)
        r["copy_census_pass_bytes_ms"] = copy_ms(G * CENSUS_B)
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
    print("\nper-launch durations of the feed's kernels (us, in launch order; the sizes in the order of the run):")
    for kn in ("k_isr_count", "k_isr_write", "k_repl_census(", "k_repl_census_sum"):
        ds = [round(x / 1e3, 1) for (x,) in c.execute("select duration from kernels where name like ? order by start", (f"%{kn}%",))]
        print(f"{kn:<20} {ds}")
    # the count pass's achieved bandwidth by grid size (one workgroup per 1024 slots), next to the copy of the same bytes
    # (which reads AND writes them) from the profiled run's own JSON lines
    copies = {}
    for f in glob.glob(os.path.join(d, "..", "profiled.json")):
        for ln in open(f):
            if ln.startswith("{"):
                r = json.loads(ln)
                copies.setdefault(r["slots"], []).append(r["copy_count_pass_bytes_ms"])
    print("\ncount pass (k_isr_count, 16 B per slot read): achieved bandwidth, best and median launch, next to (b)")
    q = "select grid_x, min(duration), count(*) from kernels where name like '%k_isr_count%' group by grid_x order by grid_x"
    try:
        rows = list(c.execute(q))
    except sqlite3.OperationalError:  # (a trace without the grid column: sizes cannot be told apart)
        rows = []
    for grid, lo, k in rows:
        G = grid // 256 * 1024 if grid % 256 == 0 else grid * 1024  # (grid_x counts work-items or workgroups, by version)
        all_ = sorted(x for (x,) in c.execute("select duration from kernels where name like '%k_isr_count%' and grid_x = ?", (grid,)))
        med = all_[len(all_) // 2]
        line = f"  {G:>9} slots: {k:>3} launches, best {lo / 1e3:7.1f} us = {G * COUNT_B / lo / 1e3:5.2f} TB/s, median {med / 1e3:7.1f} us = {G * COUNT_B / med / 1e3:5.2f} TB/s"
        for cp in copies.get(G, []):
            line += f" | copy {cp} ms = {G * COUNT_B / (cp * 1e6) / 1e3:5.2f} TB/s each way"
        print(line)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        pick = sys.argv[1] if len(sys.argv) > 1 else "all"
        sizes = [(G, R) for G in (1 << 20, 1 << 24) for R in (3, 5)]
        measure([s for s in sizes if pick == "all" or pick == f"{s[0]}x{s[1]}"])
