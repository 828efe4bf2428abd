"""jg_engine_open_groups / jg_engine_close_groups / jg_engine_list_groups at 1 M and 16 M slots (R = 3): each call timed
whole on the host (three repetitions) - a close and an open of the whole range, of a random ascending list of a quarter of
the slots, a count-only list (cap 0) and a full list - against a plain device-to-device copy of the bytes the call's
kernels touch (hipMemcpy, same device, same run).  Run under rocprofv3 by profiles/micro/vacant_groups_1m.sh; `--summarize DIR`
turns that run's kernel trace into the table of profiles/r07/vacant_groups_1m.txt."""
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

R = 3
# bytes per slot the write passes touch: a close reads the flag word and the timer record and writes every column of the
# vacant record (7 x 8 + 4 + 2 x 16 + 8 R + 3 x 8 x 8 + 8 x 4); an open loads and stores a follower lane (about 2 x 92)
CLOSE_B = 4 + 16 + 56 + 4 + 32 + 8 * R + 192 + 32
OPEN_B = 2 * (4 + 56 + 32)


def copy_ms(nbytes):
    """the best of five device-to-device copies of nbytes (hipMemcpy, timed by HIP events on the null stream)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    x, y, a, b = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(x), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(y), C.c_size_t(nbytes)) == 0
    assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0
    best = 1e9
    for _ in range(6):
        hip.hipEventRecord(a, None)
        assert hip.hipMemcpy(y, x, C.c_size_t(nbytes), 3) == 0  # hipMemcpyDeviceToDevice
        hip.hipEventRecord(b, None)
        hip.hipEventSynchronize(b)
        ms = C.c_float()
        hip.hipEventElapsedTime(C.byref(ms), a, b)
        best = min(best, ms.value)
    hip.hipFree(x), hip.hipFree(y), hip.hipEventDestroy(a), hip.hipEventDestroy(b)
    return round(best, 4)


def timed(fn, k=3):
    ts = []
    for _ in range(k):
        t0 = time.perf_counter()
        fn()
        ts.append(round(1e3 * (time.perf_counter() - t0), 3))
    return ts


def measure():
    import numpy as np
    from josefine_amd import BatchedRaft
    out = []
    for G in (1 << 20, 1 << 24):
        e = BatchedRaft(G, R, seed=1)
        rng = np.random.default_rng(G)
        sub = np.unique(rng.integers(0, G, G // 4)).astype(np.uint32)
        r = dict(slots=G, R=R, list_slots=int(sub.size))
        cl, op = [], []
        for _ in range(3):  # (close / open alternate: each call needs the other state)
            t0 = time.perf_counter()
            e.close_groups(range(G))
            cl.append(round(1e3 * (time.perf_counter() - t0), 3))
            t0 = time.perf_counter()
            e.open_groups(range(G), 100)
            op.append(round(1e3 * (time.perf_counter() - t0), 3))
        r.update(close_range_ms=cl, open_range_ms=op)
        cl, op = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            e.close_groups(sub)
            cl.append(round(1e3 * (time.perf_counter() - t0), 3))
            t0 = time.perf_counter()
            e.open_groups(sub, 200)
            op.append(round(1e3 * (time.perf_counter() - t0), 3))
        r.update(close_list_ms=cl, open_list_ms=op)
        e.close_groups(sub)
        r["count_ms"] = timed(lambda: e.count_groups())
        r["list_vacant_ms"] = timed(lambda: e.vacant_groups())
        got = e.vacant_groups()
        r["list_exact"] = bool(np.array_equal(got, sub))
        r["copy_close_bytes_ms"] = copy_ms(G * CLOSE_B)
        r["copy_open_bytes_ms"] = copy_ms(G * OPEN_B)
        r["copy_flags_ms"] = copy_ms(G * 4)
        r["download_list_bytes_ms"] = timed(lambda: got.copy(), 1)  # (a host copy, for scale)
        out.append(r)
        del e
    for r in out:
        print(json.dumps(r))


def summarize(d):
    """the kernels of a rocprofv3 run (its rocpd database) with their rate against the bytes priced per launch"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    print(f"{'kernel':<40} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        print(f"{name[:40]:<40} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f}")
    print("\nper-launch durations of the hosting kernels (us, in launch order):")
    for kn in ("k_groups_check", "k_groups_close", "k_groups_open", "k_list_count", "k_list_write", "k_scan_block_sums"):
        ds = [round(x / 1e3, 1) for (x,) in c.execute("select duration from kernels where name like ? order by start", (f"%{kn}%",))]
        print(f"{kn:<20} {ds}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        measure()
