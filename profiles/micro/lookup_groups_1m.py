"""jg_engine_lookup_groups at 1 M and 16 M slots, R = 5, every slot a leader that has replicated a few blocks: whole calls
timed on the host (best of three, all three kept) for random lists of 100, 10 k and 1 M entries and for the full range form,
with and without progress, against (a) what a caller did before ABI v16 - the same fields by whole-range read(...) plus numpy
indexing, and for the 100-entry list also per-slot read(..., g, 1) calls - and (b) a plain device-to-device copy that moves
the bytes the range form reads and writes (hipMemcpy, same device, same run).  Run under rocprofv3 by
profiles/micro/lookup_groups_1m.sh; `--summarize DIR` turns that run's kernel trace into the table of
profiles/r11/lookup_groups_1m.txt.  `--sizes G,G,...` overrides the slot counts (a dry run on the emulated device)."""
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

R = 5
READ_B = 4 + 7 * 8 + 2 * 16  # bytes per slot k_lookup loads: the flag word, seven 8-byte columns, the two cold records
ROW_B = 80                   # ... and stores: one jg_group_state (+ 8 R with progress)
FIELDS = ("term", "head", "commit", "id_gen", "election_time", "heartbeat_time", "voted_for", "leader_id", "election_timeout",
          "queued_reqs", "role", "fault", "self_slot", "repl_state", "vote_seen", "vote_granted", "has_voted", "has_leader")
VIEW = ("role", "term", "leader_id", "has_leader", "fault", "self_slot")  # what `state` / `known_leader` are made of


def best3(fn):
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        ts.append(round(1e3 * (time.perf_counter() - t0), 3))
    return dict(best=min(ts), all=ts)


def measure(sizes):
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    from josefine_amd.traces import elect_all
    from vacant_groups_1m import copy_ms
    for G in sizes:
        e = BatchedRaft(G, R, seed=1)
        elect_all(e, 10)
        acks = np.full((R, G), capi.NO_ACK, np.uint64)
        acks[0, :] = 3
        e.step_dense_acks(acks)
        acks[1:, :] = e.read("head")
        acks[0, :] = 0
        e.step_dense_acks(acks)
        e.drain_messages(), e.drain_applies(), e.drain_faults()
        rng = np.random.default_rng(G)
        r = dict(slots=G, R=R)
        r["first_lookup_ms"] = best3(lambda: e.lookup(g0=0, n=1))["all"][0]  # (allocates the staging)

        def columns(progress, index):  # (a): every field over the whole range, indexed on the host
            cols = {k: e.read(k) for k in FIELDS}
            if progress:
                cols["match"] = np.stack([e.read("match", k) for k in range(R)], axis=1)
            return {k: v[index] for k, v in cols.items()} if index is not None else cols

        def per_slot(lst, progress):  # (a'): one read per slot and field
            for g in lst:
                for k in FIELDS:
                    e.read(k, 0, int(g), 1)
                if progress:
                    for k in range(R):
                        e.read("match", k, int(g), 1)

        for n in (100, 10_000, 1_000_000):
            lst = rng.integers(0, G, n).astype(np.uint32)
            for progress in (False, True):
                tag = f"list_{n}" + ("_progress" if progress else "")
                r[f"lookup_{tag}_ms"] = best3(lambda: e.lookup(lst, progress=progress))
                r[f"columns_{tag}_ms"] = best3(lambda: columns(progress, lst))
                if n == 100:
                    r[f"per_slot_{tag}_ms"] = best3(lambda: per_slot(lst, progress))
            got, want = e.lookup(lst), columns(False, lst)
            assert all((got[k] == want[k]).all() for k in FIELDS if k in got.dtype.names), n  # the same answer
        for progress in (False, True):
            tag = "range" + ("_progress" if progress else "")
            r[f"lookup_{tag}_ms"] = best3(lambda: e.lookup(progress=progress))
            r[f"columns_{tag}_ms"] = best3(lambda: columns(progress, None))
            # (b): a copy of B bytes reads B and writes B; the range form reads READ_B and writes ROW_B (+ 8 R) per slot
            moved = READ_B + ROW_B + (8 * R if progress else 0)
            r[f"copy_{tag}_bytes_ms"] = copy_ms(G * moved // 2)
            r[f"{tag}_bytes_moved"] = G * moved
        print(json.dumps(r), flush=True)
        del e


def summarize(d):
    """the kernels of a rocprofv3 run (its rocpd database), and the lookup's kernels launch by launch"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    print(f"{'kernel':<40} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        print(f"{name[:40]:<40} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f}")
    print("\nper-launch durations of the lookup's kernels (us, in launch order; the sizes and list lengths in the order of the run):")
    for kn in ("k_lookup<", "k_lookup_check"):
        ds = [round(x / 1e3, 1) for (x,) in c.execute("select duration from kernels where name like ? order by start", (f"%{kn}%",))]
        print(f"{kn:<16} {ds}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        sizes = [1 << 20, 1 << 24]
        if len(sys.argv) > 2 and sys.argv[1] == "--sizes":
            sizes = [int(x) for x in sys.argv[2].split(",")]
        measure(sizes)
