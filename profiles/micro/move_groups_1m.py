"""jg_engine_export_groups / jg_engine_import_groups at 1 M groups (R = 5): three host-form exports and imports of an
elected engine, each timed whole on the host, against a plain copy of the same bytes in the same direction into / from
the same kind of memory (pageable numpy arrays, jg_device_download / jg_device_upload) in the same run; then the
device-form calls.  Run under rocprofv3 by profiles/micro/move_groups_1m.sh; `--summarize DIR` turns that run's kernel
trace into the table of profiles/r07/move_groups_1m_x_5.txt (kernel times and their rate against the bytes priced)."""
import ctypes as C
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

G, R = 1 << 20, 5
RECORD = 384
# the columns a record holds, per group: 7 x 8 (term .. heartbeat_time) + 4 (flags) + 32 (cold) + 32 (fvote_id)
# + 3 x 8 x 8 (window) + 8 R (match_wide)
COLUMNS = 56 + 4 + 32 + 32 + 192 + 8 * R


def measure():
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    from josefine_amd.traces import elect_all
    a = BatchedRaft(G, R, seed=3)
    elect_all(a, 10)
    acks = np.repeat(a.read("head")[None, :] + 1, R, axis=0)
    acks[0] = 1
    a.step_dense_acks(acks)
    for fn in ("drain_messages", "drain_applies", "drain_faults"):
        getattr(a, fn)()
    c = BatchedRaft(G, R, seed=3)
    nbytes = G * RECORD
    rec = np.ones(nbytes, np.uint8)
    x = capi.GroupExport()
    x.g0, x.n, x.cap_bytes, x.records = 0, G, nbytes, rec.ctypes.data
    t_exp, t_imp = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        a._check(a.api.engine_export_groups(a._h, C.byref(x)))
        t_exp.append(time.perf_counter() - t0)
    assert x.header.record_bytes == RECORD
    y = capi.GroupImport()
    y.header, y.records = x.header, rec.ctypes.data
    for _ in range(3):
        t0 = time.perf_counter()
        c._check(c.api.engine_import_groups(c._h, C.byref(y)))
        t_imp.append(time.perf_counter() - t0)
    exact = c.export_groups().records.tobytes() == rec.tobytes()
    p = C.c_void_p()
    a._check(a.api.device_alloc(a._h, nbytes, C.byref(p)))
    host = np.ones(nbytes, np.uint8)
    t_down, t_up = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        a._check(a.api.device_download(a._h, host.ctypes.data, p, nbytes))
        t_down.append(time.perf_counter() - t0)
    for _ in range(3):
        t0 = time.perf_counter()
        a._check(a.api.device_upload(a._h, p, host.ctypes.data, nbytes))
        a._check(a.api.sync(a._h))
        t_up.append(time.perf_counter() - t0)
    # the device form: records in a jg_device_alloc buffer of the same device
    xd = capi.GroupExport()
    xd.g0, xd.n, xd.flags, xd.cap_bytes, xd.records = 0, G, capi.MOVE_DEVICE, nbytes, p.value
    yd = capi.GroupImport()
    t_dexp, t_dimp = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        a._check(a.api.engine_export_groups(a._h, C.byref(xd)))
        t_dexp.append(time.perf_counter() - t0)
    yd.header, yd.flags, yd.records = xd.header, capi.MOVE_DEVICE, p.value
    for _ in range(3):
        t0 = time.perf_counter()
        c._check(c.api.engine_import_groups(c._h, C.byref(yd)))
        t_dimp.append(time.perf_counter() - t0)
    a.api.device_free(a._h, p)
    ms = lambda ts: [round(1e3 * t, 2) for t in ts]  # noqa: E731
    print(json.dumps(dict(groups=G, R=R, record_bytes=RECORD, image_bytes=nbytes, bit_exact=bool(exact),
                          export_ms=ms(t_exp), plain_download_ms=ms(t_down), export_ratio_best=round(min(t_exp) / min(t_down), 3),
                          import_ms=ms(t_imp), plain_upload_ms=ms(t_up), import_ratio_best=round(min(t_imp) / min(t_up), 3),
                          device_export_ms=ms(t_dexp), device_import_ms=ms(t_dimp))))


def summarize(d):
    """the kernels of a rocprofv3 run (its rocpd database), with the HBM rate of the three move kernels against the bytes
    priced: export and import move the records and the columns once each, the check pass reads the records"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    priced = {"k_export_groups": G * (RECORD + COLUMNS), "k_import_check": G * RECORD, "k_import_groups": G * (RECORD + COLUMNS)}
    print("kernels (all dispatches of the process):")
    print(f"{'kernel':<40} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9} {'GB/s at min':>12}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        rate = next((f"{b / lo:12.0f}" for kk, b in priced.items() if kk in name), "")
        print(f"{name[:40]:<40} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f} {rate}")
    print("\nmemory copies by size (bytes) and direction:")
    q = "select name, size, count(*), avg(duration) from memory_copies group by name, size order by size * count(*) desc"
    for name, size, k, avg in c.execute(q):
        if size * k >= 1 << 20:
            print(f"{name:<32} {size:>12} B x {k:>3}  avg {avg / 1e3:>9.1f} us  ({size / avg:.1f} GB/s)")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        measure()
