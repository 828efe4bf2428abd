"""jg_engine_read_chains at 1 M groups x 64 blocks (R = 5): three reads of a loaded engine, each timed whole on the host,
against a plain device-to-host copy of the same bytes into the same kind of destination (pageable numpy arrays,
jg_device_download) in the same run.  Run under rocprofv3 by profiles/micro/read_chains_1m.sh; `--summarize DIR` turns
that run's kernel and memory-copy traces into the table of profiles/r07/read_chains_1m_x_64.txt."""
import ctypes as C
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def image(G, n, rng, p_fork=0.2):
    """G trees of n blocks each: runs from genesis in which a block whose id is a multiple of 8 has its parent two below
    with probability p_fork (each such block starts a segment of its own: at most JG_CHAIN_WINDOW of them), and a
    "commit" key at a random block of each"""
    import numpy as np
    ids = np.tile(np.arange(n, dtype=np.uint64), G)
    nxt = np.maximum(ids.astype(np.int64) - 1, 0)
    fork = (rng.random(G * n) < p_fork) & (ids >= 2) & (ids % np.uint64(8) == 0)
    nxt = np.where(fork, ids.astype(np.int64) - 2, nxt).astype(np.uint64)
    off = np.arange(G + 1, dtype=np.uint64) * np.uint64(n)
    commit = rng.integers(1, n, G).astype(np.uint64)
    return dict(off=off, blk_id=ids, blk_next=nxt, commit=commit, has_commit=np.ones(G, np.uint8))


def measure():
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    G, R, n = 1 << 20, 5, 64
    img = image(G, n, np.random.default_rng(1))
    dev = BatchedRaft(G, R, seed=3)
    dev.load_chains(now_ms=1, **img)
    faults = len(dev.drain_faults())
    rows = G * n
    # the caller's arrays, allocated and touched once (as the plain copy's destination below)
    out = dict(off=np.ones(G + 1, np.uint64), blk_id=np.ones(rows, np.uint64), blk_next=np.ones(rows, np.uint64),
               commit=np.ones(G, np.uint64), has_commit=np.ones(G, np.uint8), fault=np.ones(G, np.uint8))
    r = capi.ChainRead()
    r.g0, r.n, r.cap = 0, G, rows
    for k, v in out.items():
        setattr(r, k, v.ctypes.data)
    got = C.c_uint64(0)
    t_read = []
    for _ in range(3):
        t0 = time.perf_counter()
        dev._check(dev.api.engine_read_chains(dev._h, C.byref(r), C.byref(got)))
        t_read.append(time.perf_counter() - t0)
    exact = bool(got.value == rows and all(np.array_equal(out[k], img[k]) for k in ("off", "blk_id", "blk_next", "commit", "has_commit")))
    # the same bytes as one plain copy: both row columns and the per-group outputs (off, commit, has_commit, fault)
    nbytes = 16 * rows + 8 * (G + 1) + 8 * G + 2 * G
    p = C.c_void_p()
    dev._check(dev.api.device_alloc(dev._h, nbytes, C.byref(p)))
    host = np.ones(nbytes, np.uint8)
    t_copy = []
    for _ in range(3):
        t0 = time.perf_counter()
        dev._check(dev.api.device_download(dev._h, host.ctypes.data, p, nbytes))
        t_copy.append(time.perf_counter() - t0)
    dev.api.device_free(dev._h, p)
    t0 = time.perf_counter()
    dev.read_chains()  # (BatchedRaft.read_chains: the sizing call, fresh numpy arrays, the read)
    t_py = time.perf_counter() - t0
    print(json.dumps(dict(groups=G, rows=rows, out_bytes=nbytes, load_faults=faults, bit_exact=exact,
                          read_ms=[round(1e3 * t, 2) for t in t_read], plain_copy_ms=[round(1e3 * t, 2) for t in t_copy],
                          ratio_best=round(min(t_read) / min(t_copy), 3), python_read_chains_ms=round(1e3 * t_py, 2))))


def summarize(d):
    """the kernels and memory copies of a rocprofv3 run (its rocpd database)"""
    import sqlite3
    db = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)[0]
    c = sqlite3.connect(db)
    print("kernels (all dispatches of the process):")
    print(f"{'kernel':<40} {'calls':>6} {'total us':>10} {'avg us':>9} {'min us':>9} {'max us':>9}")
    q = "select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels group by name order by 3 desc"
    for name, k, tot, avg, lo, hi in c.execute(q):
        print(f"{name[:40]:<40} {k:>6} {tot / 1e3:>10.1f} {avg / 1e3:>9.1f} {lo / 1e3:>9.1f} {hi / 1e3:>9.1f}")
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
