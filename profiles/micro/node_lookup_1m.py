"""Point queries in a loop of kept node steps at 1 M slots, R = 5, every slot a leader, compact bus (JG_NODE_COMMON_AE |
JG_NODE_FSM_FUSED), two ticks in flight: a lookup of 4096 random slots on every tick.  One mode per process:

  plain    no attachment: jg_step_node, the older step's outbox viewed, its rows drained by view
  looked   jg_step_node_looked on every step: the list travels with the step, the rows are viewed with the older step's outbox
  sync     what a loop could do before ABI v25: the outstanding step viewed first (the call is refused while a kept step is
           outstanding), then jg_engine_lookup_groups - one tick in flight
  calls    no loop: jg_engine_lookup_groups itself, whole calls, best of three - lists of 4096 and 65536 random slots and the
           range of all slots, with and without the progress heads

The steps carry no inbound rows (the tick's kernels, its outbox columns and fsm rows on their way home are what is timed; the
row passes are not).  Every call goes through ctypes without a host copy of the columns.  `plain`, `sync` and `calls` use
nothing ABI v25 added: the same file runs against an older tree.  Prints one JSON line.  Run by
profiles/micro/node_lookup_1m.sh; `--summarize DIR` prints the lookup kernels of a rocprofv3 --kernel-trace run, `--table FILE`
the script's part 1 as a table."""
import ctypes as C
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
N = 4096


def main(mode, slots=1 << 20, ticks=80, warmup=16):
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    from josefine_amd.traces import elect_all
    G, R = slots, 5  # (a smaller size as the second argument: a dry run)
    e = BatchedRaft(G, R, seed=1, flags=capi.CFG_SEPARATE_COMMIT_KEY)  # (a leader's Tick then scans no commit key: no Q9 fault)
    elect_all(e, 10)
    e.drain_messages(), e.drain_applies(), e.drain_faults()
    acks = np.full((R, G), capi.NO_ACK, np.uint64)
    for appends in (2, 0):  # two blocks everywhere, acknowledged by everybody a tick later: commit = head = 2
        acks[:] = capi.NO_ACK
        acks[0, :] = appends
        acks[1:, :] = e.read("head")
        e.step_dense_acks(acks)
        e.drain_messages(), e.drain_applies(), e.drain_faults()
    assert (e.read("commit") == 2).all()
    rng = np.random.default_rng(2)
    api, h = e.api, e._h

    def ok(rc):
        assert rc == capi.OK, api.error()

    if mode == "calls":
        out = {}
        for name, lst, n in (("list_4096", rng.integers(0, G, N).astype(np.uint32), N),
                             ("list_65536", rng.integers(0, G, 65536).astype(np.uint32), 65536), ("range", None, G)):
            for progress in (False, True):
                s = capi.GroupSet()
                s.n, s.flags = n, capi.LOOKUP_PROGRESS if progress else 0
                if lst is not None:
                    s.groups = lst.ctypes.data
                rows, match = np.zeros(n, capi.GROUP_STATE_DTYPE), np.zeros((n, R), np.uint64)
                ts = []
                for _ in range(4):  # (the first call sizes the staging: not counted)
                    t0 = time.perf_counter()
                    ok(api.engine_lookup_groups(h, C.byref(s), rows.ctypes.data, match.ctypes.data if progress else None))
                    ts.append(round(1e3 * (time.perf_counter() - t0), 3))
                assert (rows["head"] == 2).all() and (rows["group"] == (lst if lst is not None else np.arange(G))).all()
                out[f"lookup_{name}{'_progress' if progress else ''}_best_ms"] = min(ts[1:])
        print(json.dumps(dict(mode=mode, slots=G, R=R, **out)))
        return
    flags = capi.NODE_LEADER_HALF | capi.NODE_TICK | capi.NODE_ASYNC | capi.NODE_KEEP | capi.NODE_COMMON_AE | capi.NODE_FSM_FUSED
    outbox, total, n = capi.NodeOutbox(), C.c_size_t(0), C.c_size_t(0)
    view = capi.NodeLookup() if mode == "looked" else None
    p = C.c_void_p()
    rows = np.zeros(N, capi.GROUP_STATE_DTYPE)
    lists = [rng.integers(0, G, N).astype(np.uint32) for _ in range(warmup + ticks)]
    answered = 0

    def finish():  # the older step's outputs: its columns by view, its rows by view
        ok(api.node_outbox_view(h, C.byref(outbox)))
        ok(api.drain_applies_view(h, C.byref(p), C.byref(n)))
        ok(api.drain_messages_view(h, C.byref(p), C.byref(n)))

    def viewed(t):  # the lookup of step t: its rows are read (a checksum over the groups) where they landed
        ok(api.node_lookup_view(h, C.byref(view)))
        assert view.attached and view.n == N
        got = np.frombuffer((C.c_char * (N * 80)).from_address(view.rows), dtype=capi.GROUP_STATE_DTYPE)
        assert int(got["group"].sum()) == int(lists[t].sum())
        return 1

    times = []
    open_steps = []
    for t in range(warmup + ticks):
        t0 = time.perf_counter()
        now = 100 * (t + 1)
        if mode == "looked":
            s = capi.GroupSet()
            s.n, s.groups = N, lists[t].ctypes.data
            ok(api.step_node_looked(h, now, flags, None, None, C.byref(s)))
        else:
            ok(api.step_node(h, now, flags))
        open_steps.append(t)
        if mode == "sync":
            finish()
            open_steps.pop(0)
            s = capi.GroupSet()
            s.n, s.groups = N, lists[t].ctypes.data
            ok(api.engine_lookup_groups(h, C.byref(s), rows.ctypes.data, None))
            assert int(rows["group"].sum()) == int(lists[t].sum())
            answered += 1
        elif len(open_steps) == 2:
            finish()
            done = open_steps.pop(0)
            if mode == "looked":
                answered += viewed(done)
        times.append(time.perf_counter() - t0)
    while open_steps:
        finish()
        done = open_steps.pop(0)
        if mode == "looked":
            answered += viewed(done)
    if mode != "plain":
        assert answered == warmup + ticks, answered
    ms = np.array(times[warmup:]) * 1e3
    print(json.dumps(dict(mode=mode, slots=G, R=R, entries_per_tick=N if mode != "plain" else 0, ticks=ticks,
                          ms_per_tick_median=round(float(np.median(ms)), 3), q1=round(float(np.percentile(ms, 25)), 3),
                          q3=round(float(np.percentile(ms, 75)), 3), decisions_per_s=round(G / (float(np.median(ms)) * 1e-3), 0))))


def summarize(d):
    """the lookup kernels of a rocprofv3 --kernel-trace run (its rocpd database): launches, median, quartiles"""
    import sqlite3
    import numpy as np
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    for kn in ("k_lookup_kept<", "k_lookup<"):
        ds = np.array([x / 1e3 for (x,) in c.execute("select duration from kernels where name like ? order by start", (f"%{kn}%",))])
        if len(ds):
            print(f"{kn:<16} {len(ds)} launches: median {np.median(ds):.2f} us, quartiles {np.percentile(ds, 25):.2f} / {np.percentile(ds, 75):.2f}, "
                  f"min {ds.min():.2f}, max {ds.max():.2f}")


def table(path):
    """part 1 of node_lookup_1m.sh's output as a table: per timed line the median over each tree's runs, control / parent and
    this / parent; a line passes when this / parent is inside what the control spans: <= 1 + the largest |control / parent - 1|"""
    import numpy as np
    runs = {}
    for ln in open(path):
        f = ln.split(" ", 3)
        if len(f) < 4 or f[0] not in ("parent", "control", "this") or f[1] != "run":
            continue
        d = json.loads(ln[ln.index("{"):])
        if d["mode"] == "plain":
            rows = {"kept loop, no lookup: ms per tick": d["ms_per_tick_median"]}
        elif d["mode"] == "calls":
            rows = {f"jg_engine_lookup_groups {k[7:-8]}: ms": v for k, v in d.items() if k.startswith("lookup_")}
        else:  # (the bench: time per tick, so that larger is slower in every row)
            rows = {"bench_event_loop pipetasks compact, 2 in flight: ms per tick": d["ms_per_tick"]}
        for k, v in rows.items():
            runs.setdefault(k, {}).setdefault(f[0], []).append(v)
    med = {k: {t: float(np.median(v)) for t, v in by.items()} for k, by in runs.items()}
    span = max(abs(m["control"] / m["parent"] - 1) for m in med.values())
    print(f"== the unchanged paths (medians over the runs) - the control's largest deviation from 1: {span:.3f}")
    print(f"{'row':<66}{'parent':>9}{'control':>9}{'this':>9}  control/parent  this/parent  verdict")
    for k, m in med.items():
        c, t = m["control"] / m["parent"], m["this"] / m["parent"]
        print(f"{k:<66}{m['parent']:>9.3f}{m['control']:>9.3f}{m['this']:>9.3f}{c:>16.3f}{t:>13.3f}  {'passes' if t <= 1 + span else 'OUTSIDE'}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--table":
        table(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        main(sys.argv[1], *[int(x) for x in sys.argv[2:3]])
