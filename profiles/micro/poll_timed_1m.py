"""jg_engine_poll carrying the clock (ABI v20) against the two calls it replaces, at 1 M slots, R = 5, every slot a leader:
TWIN engines in one run, driven alike -
  two   poll(leaders, commits + backlog) followed by watch_replicas_timed: the loop of ABI v19, unchanged code
  one   poll(leaders, replicas under the time rule, commits + backlog)
Each sample is timed whole on the host, three repetitions, every one of them reported:
  quiet    every follower caught up, no clock running
  start    1 % of the followers fell silent: the sample that starts their clocks (a stamp and a mask byte stored each)
  running  their clocks run inside the window: the stamp of every such member is read
  expiry   the first sample past the window: a replicas row per slot with such a member
A repetition of the last three is one cycle: the members fall silent, start, running, expiry, then they catch up and the
rejoin is delivered (untimed).  Run under rocprofv3 by profiles/micro/poll_timed_1m.sh; `--summarize DIR` turns that run's
kernel trace into the table of profiles/r14/poll_timed_1m.txt: the timed fused count pass launch by launch against the
sum of the lag poll's fused pass over two feeds and k_isrc_count."""
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]

TWO_B, ONE_B = 84 + 17, 88 + 1  # bytes per slot the count passes read while no clock runs (DESIGN.md "One poll per tick")
WINDOW = 30_000
SAMPLES = ("quiet", "start", "running", "expiry")


def ms(t0):
    return round(1e3 * (time.perf_counter() - t0), 3)


def measure(G, R):
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    from josefine_amd.traces import elect_all
    es = [BatchedRaft(G, R, seed=1) for _ in range(2)]
    for e in es:
        elect_all(e, 10)
        e.drain_messages(), e.drain_applies(), e.drain_faults()
    rng = np.random.default_rng(6)
    down = rng.random((R, G)) < 0.01  # (member slot, slot): about 1 % of the followers
    down[0, :] = False                # (slot 0 is every leader's own)
    touched = down.any(axis=0)
    acks = np.full((R, G), capi.NO_ACK, np.uint64)
    limit = G // 10

    def tick(appends, silent):
        for e in es:
            acks[:] = e.read("head")
            acks[0, :] = appends
            if silent:
                acks[down] = capi.NO_ACK
            e.step_dense_acks(acks)
            e.drain_messages(), e.drain_applies(), e.drain_faults()

    def two(now):
        e = es[0]
        t0 = time.perf_counter()
        p = e.poll(leaders=dict(limit=limit), commits=dict(limit=limit, backlog=True))
        r = e.watch_replicas_timed(now, WINDOW, limit=limit)
        return ms(t0), (p["leaders"][1], r[1], p["commits"][1])

    def one(now):
        e = es[1]
        t0 = time.perf_counter()
        p = e.poll(leaders=dict(limit=limit), replicas=dict(now_ms=now, max_behind_ms=WINDOW, limit=limit), commits=dict(limit=limit, backlog=True))
        return ms(t0), (p["leaders"][1], p["replicas"][1], p["commits"][1])

    out = dict(slots=G, R=R, limit=limit, window_ms=WINDOW, silent_members=int(down.sum()), slots_with_one=int(touched.sum()))
    times = {s: dict(two=[], one=[]) for s in SAMPLES}
    totals = {}

    def sample(name, now, want_replicas):
        (a, ta), (b, tb) = two(now), one(now)
        assert ta == tb and ta[1] == want_replicas, (name, ta, tb, want_replicas)
        if name in times:
            times[name]["two"].append(a), times[name]["one"].append(b)
            totals[name] = list(ta)

    def drained(now):  # (everything owed delivered, in pieces of `limit`: the next sample starts from nothing)
        while any(two(now)[1]) | any(one(now)[1]):
            pass

    tick(3, False)
    tick(0, False)
    drained(1000)  # (the first look: allocates the shadows, the clocks and the staging; every slot is news)
    now = 2000
    for _ in range(3):
        now += 100
        sample("quiet", now, 0)
    for _ in range(3):
        tick(np.where(touched, 2, 0), True)
        tick(0, True)
        now += 100
        started = now
        sample("start", now, 0)
        now += 100
        sample("running", now, 0)
        now = started + WINDOW + 1
        sample("expiry", now, int(touched.sum()))
        tick(0, False)
        drained(now + 100)  # (the rejoin)
        now += 200
    for s in SAMPLES:
        out[s] = dict(two_ms=times[s]["two"], one_ms=times[s]["one"], two_best_ms=min(times[s]["two"]), one_best_ms=min(times[s]["one"]),
                      every_one_below_every_two=max(times[s]["one"]) < min(times[s]["two"]), totals_leaders_replicas_commits=totals[s])
    print(json.dumps(out), flush=True)


def summarize(d):
    """the count passes of a rocprofv3 run (its rocpd database) launch by launch"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    print(f"{'kernel':<44} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels where name like '%k_poll_count%' or name like '%k_isrc%' group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        print(f"{name[:44]:<44} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f}")
    per = {}
    for key, pat in (("fused", "%k_poll_count_timed<true, true>%"), ("lag2", "%k_poll_count<true, false, true>%"), ("isrc", "%k_isrc_count%")):
        per[key] = [round(x / 1e3, 1) for (x,) in c.execute("select duration from kernels where name like ? order by start", (pat,))]
    print("\nper-launch durations (us, in launch order; every sample launches each once: the first looks and the drains, 3 quiet,")
    print("then three cycles of start, running, expiry and the drains of the rejoin)")
    print(f"k_poll_count_timed<true, true>   {per['fused']}")
    print(f"k_poll_count<true, false, true>  {per['lag2']}")
    print(f"k_isrc_count                     {per['isrc']}")
    if len(per["lag2"]) == len(per["isrc"]):
        print(f"the sum of the last two          {[round(x + y, 1) for x, y in zip(per['lag2'], per['isrc'])]}")
    print(f"\n(quiet, one fused pass reads {ONE_B} B per slot, the two passes {TWO_B} B: {ONE_B << 20} B against {TWO_B << 20} B at 1 M slots)")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        measure(1 << 20, 5)
