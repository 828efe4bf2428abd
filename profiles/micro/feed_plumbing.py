"""Host overhead of the watch and census calls: an engine of 1 M x 3 with nothing to report, each separate call and a
poll of the three feeds 3000 times in a loop, twice; prints per call [median us, mean us] of both passes as one JSON line.
For an A/B of two builds run one process per build (JOSEFINE_GPU_LIB names the library), alternately: the table of
profiles/r15/feed_plumbing.txt."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from josefine_amd import BatchedRaft  # noqa: E402
from josefine_amd.traces import elect_all  # noqa: E402

G, R, N = 1 << 20, 3, 3000
e = BatchedRaft(G, R, seed=1)
elect_all(e, 10)
e.drain_messages(), e.drain_applies(), e.drain_faults()
calls = dict(
    leaders=lambda: e.watch_leaders(limit=64),
    leaders_count_only=lambda: e.watch_leaders(limit=0),
    census=lambda: e.census(),
    replicas=lambda: e.watch_replicas(2, 0, limit=64),
    repl_census=lambda: e.replication_census(1),
    timed=lambda: e.watch_replicas_timed(1000, 100, limit=64),
    commits=lambda: e.watch_commits(limit=64),
    commits_backlog=lambda: e.watch_commits(limit=64, backlog=True),
    poll3=lambda: e.poll(leaders=dict(limit=64), replicas=dict(leave_lag=2, join_lag=0, limit=64), commits=dict(limit=64)),
)
for f in calls.values():  # deliver everything once: quiet from here on
    e.watch_leaders(), e.watch_replicas(2, 0), e.watch_commits()
    f()
out = {}
for rep in range(2):
    for name, f in calls.items():
        ts = []
        for _ in range(N):
            t0 = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t0)
        out.setdefault(name, []).append((round(1e6 * statistics.median(ts), 2), round(1e6 * statistics.fmean(ts), 2)))
print(json.dumps(out))
