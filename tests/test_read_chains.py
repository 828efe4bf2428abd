"""jg_engine_read_chains (ABI v11): every group's chain tree read back out as the rows of a sled scan - the inverse of
jg_engine_load_chains.  The device is held to tests/ref_py: after the same fuzzed stream, each group's read equals a scan
of the RefEngine's own sled tree (ids, parents, the "commit" key).  Cases whose id contains "small" are small enough for
the emulated device (tests/test_read_chains_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, capi
from josefine_amd.engine import EngineError
from fuzz import random_batch
from parity import compare_drains, compare_snapshots
from ref_py import raft as rr
from ref_py.engine import RefEngine

pytestmark = pytest.mark.gpu

ENGINE_DOMAIN = 128  # fault codes from here on are the engine's own limits: the image is not the tree


# ---- sled trees (as tests/test_load_chains.py) -------------------------------------------------------------------
def tree_of(db, lo=0):
    """A sled scan of one tree: blocks (id, next) with id >= lo in key order, the "commit" key's value or None."""
    blocks = [(v.id, v.next) for _k, v in db.range(None, None, False) if isinstance(v, rr.Block) and v.id >= lo]
    raw = db.get(rr.COMMIT_KEY)
    return blocks, (int.from_bytes(raw, "big") if raw is not None else None)


def sled_of(tree):
    blocks, commit = tree
    db = rr.Sled()
    db.keys = [rr.block_key(i) for i, _ in blocks]
    db.map = {rr.block_key(i): rr.Block(i, nx) for i, nx in blocks}
    if commit is not None:
        db.insert(rr.COMMIT_KEY, rr.block_key(commit))
    return db


def restart_on(ref, trees, now, g0=0):
    """ref's groups g0 .. restart on `trees` (Raft::<Follower>::new + Chain::new on each)"""
    for i, t in enumerate(trees):
        ref.groups[g0 + i] = ref._new_group(g0 + i, sled_of(t), now)
        ref.fault[g0 + i] = 0
    return ref


def image_of(r):
    """the load_chains keyword arguments of a read"""
    return {k: r[k] for k in ("off", "blk_id", "blk_next", "commit", "has_commit")}


def assert_reads_equal(a, b, what=""):
    for k in ("off", "blk_id", "blk_next", "commit", "has_commit", "fault"):
        assert np.array_equal(a[k], b[k]), (what, k, np.nonzero(a[k][:len(b[k])] != b[k][:len(a[k])])[0][:8])


def assert_read_is_ref(dev, ref, what="", from_=None):
    """every group's read == ref_py's tree (filtered to ids >= from_[g]); engine-domain faults read as 0 rows"""
    G = dev.G
    trees = dev.read_trees(from_=from_)
    r = dev.read_chains(from_=from_)
    fault = dev.read("fault")
    assert np.array_equal(r["fault"], fault), what
    assert np.array_equal(np.asarray(ref.fault, np.uint8), fault), what
    for g in range(G):
        if fault[g] >= ENGINE_DOMAIN:
            assert trees[g] is None and r["off"][g] == r["off"][g + 1] and r["has_commit"][g] == 0 and r["commit"][g] == 0, (what, g)
            continue
        want = tree_of(ref.groups[g].chain.db, 0 if from_ is None else int(from_[g]))
        assert trees[g] == want, (what, g, int(fault[g]), trees[g][0][:12], want[0][:12], trees[g][1], want[1])
    return r


def continue_both(engines, ref, rng, steps, now, budget, rows, what="", between=None, compact_at=None, recreate=0.0):
    for s in range(steps):
        b = random_batch(rng, ref, rows, budget=budget)
        now += int(rng.integers(0, 300))
        rec = np.nonzero(rng.random(ref.G) < recreate)[0]
        for e in engines + [ref]:
            e.submit_columns(**b)
            for g in rec:
                e.submit(int(g), Command.Recreate())
            e.step(now)
        if s == compact_at:
            rows_c = [e.chain_compact_resident() for e in engines + [ref]]
            assert all(x.tobytes() == rows_c[-1].tobytes() for x in rows_c), what
        want = {fn: getattr(ref, fn)() for fn in ("drain_messages", "drain_applies", "drain_faults")}
        for e in engines:
            for fn, rows_w in want.items():
                got = getattr(e, fn)()
                assert got.tobytes() == rows_w.tobytes(), (what, s, fn, len(got), len(rows_w))
        if between is not None:
            between(s)
    return now


# ---- 1. against ref_py after fuzzed streams ------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,flags", [
    pytest.param(96, 1, 0, id="small-1"),
    pytest.param(96, 3, 0, id="small-3"),
    pytest.param(96, 3, capi.CFG_SEPARATE_COMMIT_KEY, id="small-3-separate"),
    pytest.param(96, 5, capi.CFG_SEPARATE_COMMIT_KEY, id="small-5-separate"),
    pytest.param(2048, 5, 0, id="2048-5"),
    pytest.param(3072, 3, capi.CFG_SEPARATE_COMMIT_KEY, id="3072-3-separate"),
])
def test_read_equals_ref_py_after_fuzzed_streams(G, R, flags):
    rng = np.random.default_rng(G + 7 * R + flags)
    kw = dict(seed=R + 11, flags=flags, self_slots=rng.integers(0, R, G).astype(np.uint8), election_timeout_ms=(300, 700))
    dev, ref = BatchedRaft(G, R, **kw), RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    reads = []
    now = continue_both([dev], ref, rng, 24, 0, budget, 3 * G if G < 1000 else 2000, compact_at=14, recreate=0.01,
                        between=lambda s: reads.append(assert_read_is_ref(dev, ref, f"step {s}")) if s % 6 == 5 else None)
    compare_snapshots(dev, ref, "stream")
    assert any(len(r["blk_id"]) for r in reads)
    assert sum(t[1] is not None for t in dev.read_trees()) >= G // 16, "the stream committed little"
    assert (dev.read("fault") > 0).any() or G < 1000 or R == 1  # (reference-domain panics occur at this size)
    # engine-domain faults: a dense ack tick asked of the groups that do not lead (JG_FAULT_ENGINE_DENSE_NONLEADER)
    acks = np.repeat(dev.read("head")[None, :], R, axis=0)
    for e in (dev, ref):
        e.step_dense_acks(acks)
    compare_drains(dev, ref, "dense acks")
    compare_snapshots(dev, ref, "dense acks")
    r = assert_read_is_ref(dev, ref, "engine faults")
    assert (r["fault"] >= ENGINE_DOMAIN).any() and (r["fault"] == 0).any()


# ---- 2. from bounds ----------------------------------------------------------------------------------------------
def random_bounds(rng, trees):
    """per group: 0, an id it holds, an id in a gap, or one above everything"""
    out = np.zeros(len(trees), np.uint64)
    for g, t in enumerate(trees):
        ids = [b[0] for b in t[0]] if t is not None else []
        k = int(rng.integers(0, 4))
        if k == 1 and ids:
            out[g] = ids[int(rng.integers(0, len(ids)))]
        elif k == 2 and ids:
            gaps = [i + 1 for a, i in zip(ids[1:], ids[:-1]) if a > i + 1]
            out[g] = gaps[int(rng.integers(0, len(gaps)))] if gaps else ids[-1] + 1
        elif k == 3:
            out[g] = (ids[-1] if ids else 0) + 1 + int(rng.integers(0, 5))
    return out


@pytest.mark.parametrize("G,R", [pytest.param(96, 3, id="small-3"), pytest.param(2048, 5, id="2048-5")])
def test_from_bounds(G, R):
    rng = np.random.default_rng(G + R)
    kw = dict(seed=4, self_slots=rng.integers(0, R, G).astype(np.uint8), election_timeout_ms=(300, 700))
    dev, ref = BatchedRaft(G, R, **kw), RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    continue_both([dev], ref, rng, 16, 0, budget, 3 * G if G < 1000 else 2000, compact_at=8)
    trees = dev.read_trees()
    for _ in range(4):
        fr = random_bounds(rng, trees)
        assert_read_is_ref(dev, ref, "from", from_=fr)
    # a sub-range with bounds
    g0, n = G // 3, G // 4
    fr = random_bounds(rng, trees[g0:g0 + n])
    sub = dev.read_chains(g0, n, fr)
    for i in range(n):
        want = tree_of(ref.groups[g0 + i].chain.db, int(fr[i]))
        got = list(zip(sub["blk_id"][sub["off"][i]:sub["off"][i + 1]].tolist(), sub["blk_next"][sub["off"][i]:sub["off"][i + 1]].tolist()))
        if dev.read("fault")[g0 + i] < ENGINE_DOMAIN:
            assert got == want[0] and (int(sub["commit"][i]) if sub["has_commit"][i] else None) == want[1], i


# ---- 3. the read has no side effects -----------------------------------------------------------------------------
def test_small_read_has_no_side_effects():
    G, R = 64, 3
    rng = np.random.default_rng(3)
    kw = dict(seed=6, self_slots=rng.integers(0, R, G).astype(np.uint8), election_timeout_ms=(300, 700))
    a, b, ref = BatchedRaft(G, R, **kw), BatchedRaft(G, R, **kw), RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)

    def between(s):
        a.read_chains()
        a.read_chains(5, 9, np.full(9, 3, np.uint64))
        compare_snapshots(a, b, f"step {s}")
        compare_snapshots(a, ref, f"step {s}")

    continue_both([a, b], ref, rng, 16, 0, budget, 3 * G, between=between, compact_at=9)
    assert_reads_equal(a.read_chains(), b.read_chains())


# ---- 4. round trip -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,flags", [pytest.param(96, 3, 0, id="small-3"),
                                       pytest.param(96, 5, capi.CFG_SEPARATE_COMMIT_KEY, id="small-5-separate"),
                                       pytest.param(4096, 5, 0, id="4096-5")])
def test_round_trip_is_a_restart(G, R, flags):
    rng = np.random.default_rng(G * R + 1)
    kw = dict(seed=8, flags=flags, self_slots=rng.integers(0, R, G).astype(np.uint8), election_timeout_ms=(300, 700))
    a, ref = BatchedRaft(G, R, **kw), RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    now = continue_both([a], ref, rng, 20, 0, budget, 3 * G if G < 1000 else 3000, compact_at=12)
    ra = a.read_chains()
    b = BatchedRaft(G, R, **kw)
    now += 100
    b.load_chains(now_ms=now, **image_of(ra))
    rb = b.read_chains()
    ok = ra["fault"] < ENGINE_DOMAIN
    assert np.array_equal(rb["fault"], np.zeros(G, np.uint8)) or not ok.all()  # (a restart clears reference-domain faults)
    for k in ("off", "blk_id", "blk_next", "commit", "has_commit"):
        assert np.array_equal(ra[k], rb[k]), k
    # b's columns == a Restart of a's groups in ref_py (a fresh RefEngine: the load's timer is the second draw, as b's)
    want = restart_on(RefEngine(G, R, **kw), [tree_of(ref.groups[g].chain.db) if ok[g] else ([], None) for g in range(G)], now)
    compare_drains(b, want, "round trip")
    compare_snapshots(b, want, "round trip")
    # ... and b goes on as the restarted reference does
    continue_both([b], want, rng, 6, now, budget, 2 * G if G < 1000 else 2000, what="after the round trip")
    compare_snapshots(b, want, "after the round trip")


# ---- 5. every storage path ---------------------------------------------------------------------------------------
def check_consistent(e, what, runs=None):
    """the read agrees with read("head") / read("commit"); where `runs` [G] is set the chain must be the run [0, head]"""
    r = e.read_chains()
    head, commit, fault = e.read("head"), e.read("commit"), e.read("fault")
    off = r["off"].astype(np.int64)
    for g in range(e.G):
        ids, nxt = r["blk_id"][off[g]:off[g + 1]], r["blk_next"][off[g]:off[g + 1]]
        assert (np.diff(ids.astype(np.float64)) > 0).all() or len(ids) < 2, (what, g)
        if fault[g] >= ENGINE_DOMAIN:
            assert len(ids) == 0 and r["has_commit"][g] == 0, (what, g)
            continue
        assert int(r["commit"][g]) == (int(commit[g]) if r["has_commit"][g] else 0), (what, g, r["commit"][g], commit[g])
        if fault[g] == 0:
            assert int(head[g]) in set(ids.tolist()), (what, g, int(head[g]), ids[:8])
        if runs is not None and runs[g]:
            h = int(head[g])
            assert np.array_equal(ids, np.arange(h + 1, dtype=np.uint64)), (what, g, h, ids[:8])
            assert np.array_equal(nxt, np.maximum(np.arange(h + 1, dtype=np.int64) - 1, 0).astype(np.uint64)), (what, g)
    # a load of it reads back identically
    twin = BatchedRaft(e.G, e.R, seed=1)
    twin.load_chains(now_ms=0, **image_of(r))
    rt = twin.read_chains()
    for k in ("off", "blk_id", "blk_next", "commit", "has_commit"):
        assert np.array_equal(r[k], rt[k]), (what, k)
    return r


def test_small_dense_ack_ticks_and_node_steps():
    from josefine_amd.traces import elect_all
    G, R = 256, 3
    dev = BatchedRaft(G, R, seed=2)
    elect_all(dev, 10)
    dev.drain_messages(), dev.drain_applies()
    for t in range(5):  # FAST leaders: the run and id_gen implicit - one append per tick, acked by both followers
        acks = np.repeat(dev.read("head")[None, :] + 1, R, axis=0)
        acks[0] = 1  # (own slot: the appends)
        dev.step_dense_acks(acks)
    assert int(dev.read("commit").min()) > 0
    check_consistent(dev, "dense acks", runs=np.ones(G, bool))
    for t in range(4):  # the node step (leader half, ticks and heartbeats)
        dev.step_node(1000 + 50 * t)
        dev.drain_messages(), dev.drain_applies()
    check_consistent(dev, "node steps", runs=np.ones(G, bool))
    # a step in flight (JG_NODE_ASYNC) is settled by the read
    dev.step_node_begin(2000, async_=True)
    r = check_consistent(dev, "async node step", runs=np.ones(G, bool))
    dev.node_outbox()
    assert len(r["blk_id"]) == int((dev.read("head") + 1).sum())


@pytest.mark.parametrize("R,vote_words", [(3, False), (5, True)])
def test_routed_cluster_rounds(R, vote_words):
    """nodes of a jg_dense_cluster with per-partition leadership (JG_CLUSTER_ANY_LEADER; R = 5 with the vote mail), read
    between routed rounds: every chain is the run [0, head] appended round by round"""
    from josefine_amd import DenseCluster as LibCluster
    from test_any_leader import spread_leaders
    G = 1200
    nodes = [BatchedRaft(G, R, seed=5 + r, self_slots=np.full(G, r, np.uint8), flags=capi.CFG_SEPARATE_COMMIT_KEY) for r in range(R)]
    spread_leaders(nodes, G, R)
    lib = LibCluster(nodes, lead=None, vote_words=vote_words)
    lib.set_appends(1)
    for t in range(12):
        lib.round_routed((t + 1) * 100)
        if t % 4 == 3:
            for n in range(R):  # a node of a cluster between rounds
                check_consistent(nodes[n], f"round {t} node {n}", runs=np.ones(G, bool))
    assert int(nodes[0].read("commit").min()) > 0
    lib.close()


# ---- 6. refusals and capacity ------------------------------------------------------------------------------------
def raw_read(e, g0, n, cap, fill=0x5A):
    bufs = dict(off=np.full(n + 1, fill, np.uint64), blk_id=np.full(max(cap, 1), fill, np.uint64),
                blk_next=np.full(max(cap, 1), fill, np.uint64), commit=np.full(max(n, 1), fill, np.uint64),
                has_commit=np.full(max(n, 1), fill, np.uint8), fault=np.full(max(n, 1), fill, np.uint8))
    r = capi.ChainRead()
    r.g0, r.n, r.cap = g0, n, cap
    r.off, r.blk_id, r.blk_next = bufs["off"].ctypes.data, bufs["blk_id"].ctypes.data, bufs["blk_next"].ctypes.data
    r.commit, r.has_commit, r.fault = bufs["commit"].ctypes.data, bufs["has_commit"].ctypes.data, bufs["fault"].ctypes.data
    rows = C.c_uint64(12345)
    rc = e.api.engine_read_chains(e._h, C.byref(r), C.byref(rows))
    return rc, rows.value, bufs


def test_small_refusals_and_capacity():
    G, R = 8, 3
    dev = BatchedRaft(G, R, seed=2)
    over = [(0, 0), (1, 0)] + [(3 + 2 * k, 1 + 2 * k) for k in range(capi.CHAIN_WINDOW + 1)]  # one segment too many
    trees = [([(0, 0), (1, 0), (2, 1), (5, 2), (6, 5)], 2), ([], None), ([(3, 2), (4, 3)], 4)] * 2 + [([(0, 0)], None), (over, 1)]
    dev.load_chains(trees, now_ms=10)
    full = dev.read_chains()
    n_rows = len(full["blk_id"])
    assert n_rows == 2 * (5 + 1 + 2) + 1 and full["fault"].tolist() == [0] * 7 + [capi.FAULT_ENGINE_WINDOW_OVERFLOW]
    # capacity: *n_rows set, nothing else written
    for cap in (0, n_rows - 1):
        rc, rows, bufs = raw_read(dev, 0, G, cap)
        assert rc == capi.ECAPACITY and rows == n_rows
        for k, v in bufs.items():
            assert (v == np.array(0x5A, v.dtype)).all(), (cap, k)
    rc, rows, bufs = raw_read(dev, 0, G, n_rows)
    assert rc == capi.OK and rows == n_rows
    for k, v in full.items():
        assert np.array_equal(bufs[k][:len(v)], v), k
    rc, rows, bufs = raw_read(dev, 2, 3, 0)  # groups 2, 3, 4: 2 + 5 + 1 rows
    assert rc == capi.ECAPACITY and rows == 8
    rc, rows, bufs = raw_read(dev, 7, 1, 0)  # an engine-faulted group has no rows: cap 0 reads it
    assert rc == capi.OK and rows == 0 and bufs["off"][:2].tolist() == [0, 0] and bufs["has_commit"][0] == 0
    assert bufs["fault"][0] == capi.FAULT_ENGINE_WINDOW_OVERFLOW and bufs["commit"][0] == 0
    # the range outside G
    for g0, n in ((G - 1, 2), (G, 1), (0, G + 1)):
        rc, _, bufs = raw_read(dev, g0, n, 64)
        assert rc == capi.EINVAL and (bufs["off"] == 0x5A).all(), (g0, n)
    # kept node steps outstanding
    dev.step_node_begin(30, async_=True, keep=True)
    rc, _, bufs = raw_read(dev, 0, G, 64)
    assert rc == capi.EINVAL and (bufs["blk_id"] == 0x5A).all()
    with pytest.raises(EngineError):
        dev.read_chains()
    dev.node_outbox()
    dev.drain_messages(), dev.drain_applies(), dev.drain_faults()
    # queued commands are not in the image
    dev.submit(0, Command.AppendEntries(1, 2, [(7, 6)]))
    assert_reads_equal(dev.read_chains(), full, "queued")
    dev.step(40)
    assert (7, 6) in dev.read_trees()[0][0]


# ---- 7. skew, full size, several shards (GPU only) ---------------------------------------------------------------
def test_one_huge_tree_among_small_ones():
    n = 1_000_000
    ids = np.arange(n, dtype=np.uint64)
    nxt = np.maximum(ids.astype(np.int64) - 1, 0).astype(np.uint64)
    for at in (1000, 250_000, 999_000):
        nxt[at] = at - 2
    big = (list(zip(ids.tolist(), nxt.tolist())), 600_000)
    trees = [([(0, 0), (1, 0), (2, 1)], 2), big, ([(0, 0), (1, 0), (4, 1)], 4), ([], None), ([(9, 3)], None)]
    dev = BatchedRaft(8, 3, seed=1)
    dev.load_chains(trees, now_ms=5, g0=1)
    got = dev.read_trees(1, 5)
    want = [([(0, 0)] if t[1] is None and (not t[0] or t[0][0][0] != 0) else []) for t in trees]  # (Chain::new's genesis)
    for i, t in enumerate(trees):
        blocks = sorted(set(t[0]) | set(want[i]))
        assert got[i] == (blocks, t[1]), i
    fr = np.array([0, 999_500, 3, 0, 10], np.uint64)
    sub = dev.read_trees(1, 5, fr)
    assert sub[1][0] == [b for b in got[1][0] if b[0] >= 999_500] and sub[1][1] == 600_000


def test_full_size_round_trip_and_shards():
    from test_load_chains import random_image
    G, R = 1 << 20, 5
    rng = np.random.default_rng(11)
    img, grp, k = random_image(G, rng, mean=64)
    assert len(img["blk_id"]) > 3 * (1 << 24)  # several staging pieces
    a = BatchedRaft(G, R, seed=3)
    a.load_chains(now_ms=1, **img)
    ra = a.read_chains()
    bad = ra["fault"] >= ENGINE_DOMAIN
    assert bad.any() and not bad.all()
    # bit-exact: the healthy groups' rows are the image's - plus Chain::new's genesis where the commit is 0 and block 0 is
    # not stored (chain.rs:132-153) - and the faulted ones have none
    off = img["off"].astype(np.int64)
    n_img = np.diff(off)
    c = np.where(img["has_commit"] == 1, img["commit"], 0)
    first = img["blk_id"][np.minimum(off[:-1], len(img["blk_id"]) - 1)]
    add = ~bad & (c == 0) & ((n_img == 0) | (first != 0))
    at = off[:-1][add]
    ids = np.insert(img["blk_id"], at, 0)
    nxt = np.insert(img["blk_next"], at, 0)
    keep = ~bad[np.insert(grp, at, np.nonzero(add)[0])]
    assert np.array_equal(np.diff(ra["off"].astype(np.int64)), np.where(bad, 0, n_img + add))
    assert np.array_equal(ra["blk_id"], ids[keep]) and np.array_equal(ra["blk_next"], nxt[keep])
    assert np.array_equal(ra["commit"], np.where(bad | (img["has_commit"] == 0), 0, img["commit"]))
    assert np.array_equal(ra["has_commit"], np.where(bad, 0, img["has_commit"]))
    b = BatchedRaft(G, R, seed=3)
    b.load_chains(now_ms=1, **image_of(ra))
    rb = b.read_chains()
    # (an engine-faulted group was read as an empty tree: it loads as one, Chain::new's genesis alone)
    at = ra["off"][:-1][bad].astype(np.int64)
    assert np.array_equal(np.diff(rb["off"].astype(np.int64)), np.diff(ra["off"].astype(np.int64)) + bad)
    assert np.array_equal(rb["blk_id"], np.insert(ra["blk_id"], at, 0)) and np.array_equal(rb["blk_next"], np.insert(ra["blk_next"], at, 0))
    assert np.array_equal(ra["commit"], rb["commit"]) and np.array_equal(ra["has_commit"], rb["has_commit"]) and not rb["fault"].any()
    fr = np.where(rng.random(G) < 0.5, rng.integers(0, 80, G), 0).astype(np.uint64)
    one = a.read_chains(from_=fr)
    del b, rb
    for D in (2, 3):
        s = BatchedRaft(G, R, seed=3, device_ids=[0] * D)
        s.load_chains(now_ms=1, **img)
        assert_reads_equal(s.read_chains(), ra, f"{D} shards")
        assert_reads_equal(s.read_chains(from_=fr), one, f"{D} shards, from")
        g0, n = G // 3 - 5, G // 2
        assert_reads_equal(s.read_chains(g0, n), a.read_chains(g0, n), f"{D} shards, a range")
        del s
