"""Hosting in a loop of kept node steps at 1 M slots, R = 5, every slot a leader at first, compact bus (JG_NODE_COMMON_AE |
JG_NODE_FSM_FUSED), two ticks in flight: on every tick a close of 4096 listed slots and an open of the 4096 closed a tick
earlier.  One mode per process:

  plain    no attachment: jg_step_node, the older step's outbox viewed, its rows drained by view
  hosted   jg_step_node_hosted on every step: the two lists travel with the step, the verdict is viewed with the older step's
           outbox
  sync     what a loop could do before ABI v26: the outstanding step viewed first (the calls are refused while a kept step is
           outstanding), then jg_engine_close_groups and jg_engine_open_groups - one tick in flight
  calls    no loop: jg_engine_close_groups / jg_engine_open_groups themselves, whole calls, best of three - a list of 4096
           slots and the range of all slots

The steps carry no inbound rows (the tick's kernels, its outbox columns and fsm rows on their way home are what is timed; the
row passes are not).  Every call goes through ctypes.  `plain`, `sync` and `calls` use nothing ABI v26 added: the same file
runs against an older tree.  Prints one JSON line.  Run by profiles/micro/node_hosting_1m.sh; `--summarize DIR` prints the
hosting kernels of a rocprofv3 --kernel-trace run, `--table FILE` the script's part 1 as a table."""
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
    e = BatchedRaft(G, R, seed=1, flags=capi.CFG_SEPARATE_COMMIT_KEY)
    elect_all(e, 10)
    e.drain_messages(), e.drain_applies(), e.drain_faults()
    rng = np.random.default_rng(2)
    api, h = e.api, e._h

    def ok(rc):
        assert rc == capi.OK, api.error()

    def a_set(lst=None, n=0):
        s = capi.GroupSet()
        s.n = n if lst is None else len(lst)
        if lst is not None:
            s.groups = lst.ctypes.data
        return s

    if mode == "calls":
        out = {}
        lst = np.sort(rng.choice(G, N, replace=False)).astype(np.uint32)
        for name, s in (("list_4096", a_set(lst)), ("range", a_set(n=G))):
            tc, to = [], []
            for k in range(4):  # (the first pair sizes the staging: not counted)
                t0 = time.perf_counter()
                ok(api.engine_close_groups(h, C.byref(s)))
                t1 = time.perf_counter()
                ok(api.engine_open_groups(h, 100 * (k + 1), C.byref(s)))
                t2 = time.perf_counter()
                tc.append(round(1e3 * (t1 - t0), 3)), to.append(round(1e3 * (t2 - t1), 3))
            out[f"close_{name}_best_ms"], out[f"open_{name}_best_ms"] = min(tc[1:]), min(to[1:])
        assert len(e.vacant_groups()) == 0
        print(json.dumps(dict(mode=mode, slots=G, R=R, **out)))
        return
    flags = capi.NODE_LEADER_HALF | capi.NODE_TICK | capi.NODE_ASYNC | capi.NODE_KEEP | capi.NODE_COMMON_AE | capi.NODE_FSM_FUSED
    outbox, n = capi.NodeOutbox(), C.c_size_t(0)
    p = C.c_void_p()
    T = warmup + ticks
    assert (T + 1) * N <= G or slots != 1 << 20
    per = min(N, G // (T + 1))
    perm = rng.permutation(G)[:(T + 1) * per].reshape(T + 1, per)
    lists = [np.sort(c).astype(np.uint32) for c in perm]  # (list t is closed by tick t and opened by tick t + 1)
    answered = 0

    def finish():  # the older step's outputs: its columns by view, its rows by view
        ok(api.node_outbox_view(h, C.byref(outbox)))
        ok(api.drain_applies_view(h, C.byref(p), C.byref(n)))
        ok(api.drain_messages_view(h, C.byref(p), C.byref(n)))

    def viewed(t):
        v = capi.NodeHosting()
        ok(api.node_hosting_view(h, C.byref(v)))
        assert (v.attached, v.state, v.closed, v.opened) == (1, 0, per, per if t else 0), (t, v.state, v.closed, v.opened)
        return 1

    times = []
    open_steps = []
    for t in range(T):
        t0 = time.perf_counter()
        now = 100 * (t + 1)
        close, opened = a_set(lists[t]), a_set(lists[t - 1]) if t else None
        if mode == "hosted":
            r = capi.NodeHostingRequest()
            r.close, r.open = C.addressof(close), C.addressof(opened) if t else None
            ok(api.step_node_hosted(h, now, flags, None, None, None, C.byref(r)))
        else:
            ok(api.step_node(h, now, flags))
        open_steps.append(t)
        if mode == "sync":
            finish()
            open_steps.pop(0)
            ok(api.engine_close_groups(h, C.byref(close)))
            if t:
                ok(api.engine_open_groups(h, now, C.byref(opened)))
            answered += 1
        elif len(open_steps) == 2:
            finish()
            done = open_steps.pop(0)
            if mode == "hosted":
                answered += viewed(done)
        times.append(time.perf_counter() - t0)
    while open_steps:
        finish()
        done = open_steps.pop(0)
        if mode == "hosted":
            answered += viewed(done)
    if mode != "plain":
        assert answered == T, answered
        assert np.array_equal(e.vacant_groups(), lists[T - 1])
    ms = np.array(times[warmup:]) * 1e3
    print(json.dumps(dict(mode=mode, slots=G, R=R, closed_and_opened_per_tick=per if mode != "plain" else 0, ticks=ticks,
                          ms_per_tick_median=round(float(np.median(ms)), 3), q1=round(float(np.percentile(ms, 25)), 3),
                          q3=round(float(np.percentile(ms, 75)), 3), decisions_per_s=round(G / (float(np.median(ms)) * 1e-3), 0))))


def summarize(d):
    """the hosting kernels of a rocprofv3 --kernel-trace run (its rocpd database): launches, median, quartiles"""
    import sqlite3
    import numpy as np
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    for kn in ("k_groups_check_kept", "k_groups_close_kept", "k_groups_open_kept"):
        ds = np.array([x / 1e3 for (x,) in c.execute("select duration from kernels where name like ? order by start", (f"%{kn}%",))])
        if len(ds):
            print(f"{kn:<20} {len(ds)} launches: median {np.median(ds):.2f} us, quartiles {np.percentile(ds, 25):.2f} / {np.percentile(ds, 75):.2f}, "
                  f"min {ds.min():.2f}, max {ds.max():.2f}")


def table(path):
    """part 1 of node_hosting_1m.sh's output as a table: per timed line the median over each tree's runs, control / parent and
    this / parent; a line passes when this / parent is inside what the control spans: within the largest |control / parent - 1|
    of 1, on either side (a path that is not meant to change and got much faster is as much a finding as one that got slower)"""
    import numpy as np
    runs = {}
    for ln in open(path):
        f = ln.split(" ", 3)
        if len(f) < 4 or f[0] not in ("parent", "control", "this") or f[1] != "run":
            continue
        d = json.loads(ln[ln.index("{"):])
        if d["mode"] == "plain":
            rows = {"kept loop, no attachment: ms per tick": d["ms_per_tick_median"]}
        elif d["mode"] == "calls":
            rows = {f"jg_engine_{k.split('_')[0]}_groups {k[k.index('_') + 1:-8]}: ms": v for k, v in d.items() if k.endswith("_best_ms")}
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
        print(f"{k:<66}{m['parent']:>9.3f}{m['control']:>9.3f}{m['this']:>9.3f}{c:>16.3f}{t:>13.3f}  {'passes' if abs(t - 1) <= span else 'OUTSIDE'}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--table":
        table(sys.argv[2])
    elif len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        main(sys.argv[1], *[int(x) for x in sys.argv[2:3]])
