"""jg_engine_load_chains (ABI v10): an engine opened on the sled trees a restarting process left behind - Raft::<Follower>::new
+ Chain::new for every group of a range (follower.rs:68-95, chain.rs:117-137).  The device is held to tests/ref_py: the
expected engine is a RefEngine whose groups are re-made by `_new_group` on copies of the same trees, which is that very
constructor over sled.  Cases whose id contains "small" are small enough for the emulated device
(tests/test_load_chains_emulated.py)."""
import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, capi
from josefine_amd.engine import EngineError
from fuzz import random_batch
from parity import compare_drains, compare_snapshots
from ref_py import raft as rr
from ref_py.engine import RefEngine

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1


# ---- sled trees ------------------------------------------------------------------------------------------------------
def tree_of(db):
    """A sled scan of one tree: blocks (id, next) in key order, the "commit" key's value or None."""
    blocks = [(v.id, v.next) for _k, v in db.range(None, None, False) if isinstance(v, rr.Block)]
    raw = db.get(rr.COMMIT_KEY)
    return blocks, (int.from_bytes(raw, "big") if raw is not None else None)


def sled_of(tree):
    blocks, commit = tree
    db = rr.Sled()
    db.keys = [rr.block_key(i) for i, _ in blocks]  # (ascending ids: sled's key order already)
    db.map = {rr.block_key(i): rr.Block(i, nx) for i, nx in blocks}
    if commit is not None:
        db.insert(rr.COMMIT_KEY, rr.block_key(commit))
    return db


def expected(G, R, trees, now, g0=0, ref=None, **kw):
    """RefEngine whose groups g0 .. g0 + len(trees) - 1 restart on `trees` (a fresh one unless `ref` is given)"""
    ref = RefEngine(G, R, **kw) if ref is None else ref
    for i, t in enumerate(trees):
        ref.groups[g0 + i] = ref._new_group(g0 + i, sled_of(t), now)
        ref.fault[g0 + i] = 0
    return ref


def csr(trees):
    off = np.zeros(len(trees) + 1, np.uint64)
    off[1:] = np.cumsum([len(t[0]) for t in trees])
    ids = np.array([b[0] for t in trees for b in t[0]], dtype=np.uint64)
    nxt = np.array([b[1] for t in trees for b in t[0]], dtype=np.uint64)
    commit = np.array([t[1] or 0 for t in trees], dtype=np.uint64)
    has = np.array([t[1] is not None for t in trees], dtype=np.uint8)
    return dict(off=off, blk_id=ids, blk_next=nxt, commit=commit, has_commit=has)


def continue_both(dev, ref, rng, steps, now, budget, rows=300, what=""):
    """the same random stream into both, drains and every column compared after every step"""
    for s in range(steps):
        b = random_batch(rng, ref, rows, budget=budget)
        now += int(rng.integers(0, 300))
        for e in (dev, ref):
            e.submit_columns(**b)
            e.step(now)
        compare_drains(dev, ref, f"{what} continued step {s}")
        compare_snapshots(dev, ref, f"{what} continued step {s}")
    return now


# ---- 1. differential against the independent restatement -----------------------------------------------------------
@pytest.mark.parametrize("G,R,flags,steps", [
    pytest.param(96, 3, 0, 12, id="small-3"),
    pytest.param(96, 5, capi.CFG_SEPARATE_COMMIT_KEY, 12, id="small-5-separate"),
    pytest.param(2048, 1, capi.CFG_SEPARATE_COMMIT_KEY, 100, id="2048-1-separate"),
    pytest.param(3072, 3, 0, 100, id="3072-3"),
    pytest.param(2048, 5, capi.CFG_SEPARATE_COMMIT_KEY, 100, id="2048-5-separate"),
    pytest.param(4096, 5, 0, 100, id="4096-5"),
])
def test_load_equals_ref_py_restart_on_the_same_trees(G, R, flags, steps):
    rng = np.random.default_rng(G + 10 * R + flags)
    kw = dict(seed=R + 3, flags=flags, self_slots=rng.integers(0, R, G).astype(np.uint8), election_timeout_ms=(300, 700))
    # the trees: a fuzzed stream (forks, gaps, re-sent blocks, restarts, elections) and a compaction, on ref_py alone
    src = RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    now = 0
    for s in range(30):
        src.submit_columns(**random_batch(rng, src, 4 * G, budget=budget))
        now += int(rng.integers(0, 300))
        src.step(now)
        if s == 20:
            src.chain_compact_resident()
    src.drain_messages(), src.drain_applies(), src.drain_faults()
    trees = [tree_of(src.groups[g].chain.db) for g in range(G)]
    assert any(t[1] is None for t in trees) or flags  # (both kinds of tree occur)
    assert sum(len(t[0]) for t in trees) > 5 * G and sum(t[1] is not None and t[1] > 0 for t in trees) > G // 8, "the stream built little"

    dev = BatchedRaft(G, R, **kw)
    ref = RefEngine(G, R, **kw)
    compare_snapshots(dev, ref, "fresh")  # one draw spent per group on both sides ...
    assert ref.draws == [1] * G
    now += 50
    dev.load_chains(trees, now_ms=now)
    expected(G, R, trees, now, ref=ref)
    assert ref.draws == [2] * G  # ... and the load's timer is the second on both
    compare_drains(dev, ref, "load")
    compare_snapshots(dev, ref, "load")
    now = continue_both(dev, ref, rng, steps, now, budget, rows=2 * G if G < 1000 else 400)
    a, b = dev.chain_compact_resident(), ref.chain_compact_resident()  # the walk over the loaded parent pointers
    assert a.tobytes() == b.tobytes(), (len(a), len(b))
    compare_snapshots(dev, ref, "compacted")


# ---- 2. edge cases ------------------------------------------------------------------------------------------------
def run_case(trees, G=8, R=3, g0=0, steps=6, now=1000, flags=0, stream=True, budget=2):
    kw = dict(seed=5, flags=flags)
    dev = BatchedRaft(G, R, **kw)
    dev.load_chains(trees, now_ms=now, g0=g0)
    ref = expected(G, R, trees, now, g0=g0, **kw)
    compare_drains(dev, ref, "load")
    compare_snapshots(dev, ref, "load")
    if stream:
        continue_both(dev, ref, np.random.default_rng(len(trees) + g0), steps, now, np.full(G, budget),
                      rows=4 * G)
    return dev, ref


RUN = [(0, 0), (1, 0), (2, 1), (3, 2), (4, 3)]
EDGE = {
    "empty": ([], None),
    "genesis": ([(0, 0)], None),
    "commit0": (RUN, 0),
    "nokey": (RUN, None),
    "commit": (RUN + [(5, 4), (6, 5)], 4),
    "nogenesis": ([(3, 2), (4, 3), (5, 4), (9, 4)], 5),
    "nogenesis-nokey": ([(3, 2), (4, 3)], None),
    "gaps": ([(0, 0), (1, 0), (2, 1), (5, 2), (6, 5), (7, 6), (8, 1), (12, 11), (13, 12)], 7),
}


@pytest.mark.parametrize("case", sorted(EDGE))
def test_small_edge_trees(case):
    trees = [EDGE[case], ([(0, 0), (1, 0)], 1), EDGE[case]]
    run_case(trees, G=6, g0=1)


def test_small_empty_tree_is_recreate():
    dev, _ = run_case([([], None)] * 4, G=4, stream=False)
    twin = BatchedRaft(4, 3, seed=5)
    twin.apply_all(Command.Recreate(), 1000)
    compare_snapshots(dev, twin, "empty tree vs JG_CMD_RECREATE")


def window_tree(extra):
    """genesis run [0, 1] and `extra` more segments (forks: next = id - 2)"""
    blocks = [(0, 0), (1, 0)] + [(3 + 2 * k, 1 + 2 * k) for k in range(extra)]
    return blocks, blocks[-1][0]


def test_small_window_full_loads():
    assert len(window_tree(capi.CHAIN_WINDOW)[0]) == capi.CHAIN_WINDOW + 2
    dev, ref = run_case([window_tree(capi.CHAIN_WINDOW), window_tree(3)], G=4, stream=False)
    assert not dev.read("fault").any()
    continue_both(dev, ref, np.random.default_rng(8), 6, 1000, np.zeros(4, np.int64), rows=16)  # (no budget: no new segment)


def test_small_window_overflow_faults_that_group_only():
    G, R, now = 6, 3, 700
    trees = [window_tree(3), window_tree(capi.CHAIN_WINDOW + 1), window_tree(capi.CHAIN_WINDOW)]
    dev = BatchedRaft(G, R, seed=5)
    dev.load_chains(trees, now_ms=now, g0=2)
    f = dev.drain_faults()
    assert [(int(r["group"]), int(r["code"])) for r in f] == [(3, capi.FAULT_ENGINE_WINDOW_OVERFLOW)]
    ref = expected(G, R, trees, now, g0=2, seed=5)
    ok = [g for g in range(G) if g != 3]
    for name in capi.FIELD_NAMES:
        if name == "match":
            continue
        a, b = dev.read(name), ref.read(name)
        assert np.array_equal(a[ok], b[ok]), name
    assert dev.read("fault")[3] == capi.FAULT_ENGINE_WINDOW_OVERFLOW
    # a restart of the faulted group clears the fault (the stored tree it restarts on is the device's own)
    dev.apply(3, Command.Restart(), now)
    assert dev.read("fault")[3] == 0


def test_small_genesis_with_a_parent_faults():
    dev = BatchedRaft(4, 3, seed=5)
    dev.load_chains([([(0, 7), (1, 0)], 1), ([(0, 0)], None)], now_ms=5)
    assert [(int(r["group"]), int(r["code"])) for r in dev.drain_faults()] == [(0, capi.FAULT_ENGINE_WINDOW_OVERFLOW)]
    assert dev.read("fault").tolist() == [capi.FAULT_ENGINE_WINDOW_OVERFLOW, 0, 0, 0]


def test_small_ids_near_the_top():
    top = [(0, 0), (1, 0), ((1 << 56) - 1, 1), (1 << 56, (1 << 56) - 1), (M64 - 1, 1 << 56), (M64, M64 - 1)]
    dev, ref = run_case([(top, 1 << 56), (top, M64), (top[2:], None)], G=4, stream=False)
    for e in (dev, ref):  # a block on top of the committed one, then its commit
        e.submit(0, Command.AppendEntries(1, 2, [((1 << 56) + 1, 1 << 56)]))
        e.submit(0, Command.Heartbeat(1, (1 << 56) + 1, 2))
        e.submit(1, Command.AppendEntries(1, 2, [(5, 1)]))
        e.step(2000)
    compare_drains(dev, ref, "near the top")
    compare_snapshots(dev, ref, "near the top")
    assert int(dev.read("commit")[0]) == (1 << 56) + 1 and int(dev.read("head")[1]) == 5


def test_small_range_leaves_the_other_groups_alone():
    G, R = 24, 3
    kw = dict(seed=9, election_timeout_ms=(300, 700))
    dev, ref = BatchedRaft(G, R, **kw), RefEngine(G, R, **kw)
    rng = np.random.default_rng(4)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    now = continue_both(dev, ref, rng, 8, 0, budget, rows=6 * G, what="before")
    before = dev.snapshot()
    trees = [tree_of(ref.groups[g].chain.db) for g in range(5, 12)]
    dev.load_chains(trees, now_ms=now + 1, g0=5)
    expected(G, R, trees, now + 1, g0=5, ref=ref)
    compare_drains(dev, ref, "range load")
    compare_snapshots(dev, ref, "range load")
    after = dev.snapshot()
    out = np.r_[0:5, 12:G]
    for name, col in before.items():
        assert np.array_equal(col[..., out], after[name][..., out]), name
    continue_both(dev, ref, rng, 8, now + 1, budget, rows=6 * G, what="after")


def refusal(dev, what, fn):
    before = dev.snapshot()
    with pytest.raises(EngineError):
        fn()
    after = dev.snapshot()
    for name, col in before.items():
        assert np.array_equal(col, after[name]), (what, name)
    assert len(dev.drain_faults()) == 0, what


def test_small_refusals_change_nothing():
    G, R = 8, 3
    dev = BatchedRaft(G, R, seed=2)
    dev.load_chains([(RUN, 3)] * G, now_ms=10)
    dev.drain_faults()
    good = csr([(RUN, 2), ([(0, 0), (1, 0)], 1)])

    def load(**over):
        a = dict(good, **over)
        return lambda g0=0: dev.load_chains(now_ms=99, g0=g0, **a)
    refusal(dev, "off[0] != 0", load(off=np.array([1, 5, 7], np.uint64)))
    refusal(dev, "off not monotone", load(off=np.array([0, 5, 4], np.uint64)))
    refusal(dev, "range outside G", lambda: load()(g0=G - 1))
    # ids not strictly ascending: found on the device, in the second group, after a good first one
    refusal(dev, "descending", load(blk_id=np.array([0, 1, 2, 3, 4, 1, 0], np.uint64)))
    refusal(dev, "repeated id", load(blk_id=np.array([0, 1, 2, 2, 4, 0, 1], np.uint64)))
    # commands submitted and not stepped
    dev.submit(0, Command.Tick())
    refusal(dev, "queued commands", load())
    dev.step(20)
    # a kept node step (JG_NODE_KEEP) outstanding
    dev.step_node_begin(30, async_=True, keep=True)
    refusal(dev, "kept node step", load())
    dev.node_outbox()
    dev.drain_messages(), dev.drain_applies(), dev.drain_faults()
    load()()  # and then it loads
    assert int(dev.read("commit")[0]) == 2


def test_one_huge_tree_among_small_ones():
    n = 1_000_000
    ids = np.arange(n, dtype=np.uint64)
    nxt = np.maximum(ids.astype(np.int64) - 1, 0).astype(np.uint64)
    for at in (1000, 250_000, 999_000):  # three forks: next two below
        nxt[at] = at - 2
    big = (list(zip(ids.tolist(), nxt.tolist())), 600_000)
    trees = [(RUN, 2), big, ([(0, 0), (1, 0), (4, 1)], 4), ([], None)]
    run_case(trees, G=6, g0=1, steps=4)


# ---- 3. full size ------------------------------------------------------------------------------------------------
def mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def random_image(G, rng, mean=32):
    """G trees of ~mean blocks: runs from genesis with forks (next two below) and gaps (a parent further down), some with
    block 0 compacted away, some without a commit key; CSR arrays"""
    n = rng.integers(0, 2 * mean, G)
    off = np.zeros(G + 1, np.uint64)
    off[1:] = np.cumsum(n)
    N = int(off[-1])
    grp = np.repeat(np.arange(G), n)
    k = np.arange(N) - off[grp].astype(np.int64)  # position within the tree
    step = np.where(rng.random(N) < 0.05, 2, 1)  # gaps in the ids
    step[off[:-1][n > 0].astype(np.int64)] = 0
    start = np.where(rng.random(G) < 0.1, rng.integers(1, 50, G), 0)  # block 0 compacted away
    ids = (np.cumsum(step) - np.cumsum(step)[off[grp].astype(np.int64)] + start[grp]).astype(np.uint64)
    nxt = np.where(k == 0, 0, ids.astype(np.int64) - 1)
    fork = (rng.random(N) < 0.04) & (k >= 2)
    nxt = np.where(fork, ids.astype(np.int64) - 3, nxt)
    nxt = np.where((start[grp] > 0) & (k == 0), ids.astype(np.int64) - 1, nxt).astype(np.uint64)
    has = (rng.random(G) < 0.8).astype(np.uint8)
    last = np.where(n > 0, ids[np.maximum(off[1:].astype(np.int64) - 1, 0)], 0)
    commit = np.where(has == 1, (last * rng.random(G)).astype(np.uint64), 0).astype(np.uint64)
    return dict(off=off, blk_id=ids, blk_next=nxt, commit=commit, has_commit=has), grp, k


def chain_new_columns(img, grp, k, G, R, now, seed, el=(500, 1000)):
    """numpy statement of Chain::new + Raft::<Follower>::new for every group (second timer draw) and of the faults"""
    ids, nxt, off = img["blk_id"].astype(np.int64), img["blk_next"].astype(np.int64), img["off"].astype(np.int64)
    prev = np.r_[-2, ids[:-1]]
    start = (k == 0) | (ids != prev + 1) | (nxt != ids - 1)
    nseg = np.bincount(grp, weights=start, minlength=G).astype(np.int64)
    n = off[1:] - off[:-1]
    gen = (n > 0) & (ids[np.minimum(off[:-1], len(ids) - 1)] == 0)
    extra = nseg - gen
    fault = np.where(extra > capi.CHAIN_WINDOW, capi.FAULT_ENGINE_WINDOW_OVERFLOW, 0)
    c = np.where(img["has_commit"] == 1, img["commit"], 0).astype(np.uint64)
    key = np.arange(G, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95) + np.uint64(1)
    r = mix64(np.uint64(seed) ^ mix64(key))
    timeout = (el[0] + r % np.uint64(el[1] - el[0])).astype(np.uint32)
    return dict(commit=c, head=c, id_gen=np.where(c == 0, 1, c).astype(np.uint64), term=np.zeros(G, np.uint64),
                role=np.zeros(G, np.uint8), fault=fault.astype(np.uint8), election_time=np.full(G, now, np.uint64),
                election_timeout=timeout, voted_for=np.zeros(G, np.uint32), leader_id=np.zeros(G, np.uint32),
                heartbeat_time=np.zeros(G, np.uint64), queued_reqs=np.zeros(G, np.uint32))


def test_full_size_load():
    G, R, now, seed = 1 << 20, 5, 777, 3
    rng = np.random.default_rng(1)
    img, grp, k = random_image(G, rng)
    dev = BatchedRaft(G, R, seed=seed)
    dev.load_chains(now_ms=now, **img)
    want = chain_new_columns(img, grp, k, G, R, now, seed)
    f = dev.drain_faults()
    assert np.array_equal(np.sort(f["group"]), np.nonzero(want["fault"])[0])
    for name, col in want.items():
        got = dev.read(name)
        assert np.array_equal(got, col), (name, np.nonzero(got != col)[0][:8])
    # Chain::compact of the resident chains == the pure function over the image (k_chain_compact)
    removed = np.zeros(len(img["blk_id"]), np.uint8)
    c = np.where(want["fault"] == 0, want["commit"], 0).astype(np.uint64)  # (faulted groups are not compacted)
    dev._check(dev.api.chain_compact(dev._h, G, img["off"].ctypes.data, img["blk_id"].ctypes.data,
                                     img["blk_next"].ctypes.data, c.ctypes.data, removed.ctypes.data))
    rows = dev.chain_compact_resident()
    gi = np.nonzero(removed)[0]
    order = np.lexsort((-img["blk_id"][gi].astype(np.float64), grp[gi]))  # group ascending, ids descending (the walk)
    assert np.array_equal(rows["group"], grp[gi][order]) and np.array_equal(rows["id"], img["blk_id"][gi][order])
    # the same load through a two-shard handle
    two = BatchedRaft(G, R, seed=seed, device_ids=[0, 0])
    two.load_chains(now_ms=now, **img)
    assert np.array_equal(np.sort(two.drain_faults()["group"]), np.sort(f["group"]))
    fresh = BatchedRaft(G, R, seed=seed)
    fresh.load_chains(now_ms=now, **img)
    fresh.drain_faults()
    compare_snapshots(two, fresh, "two shards vs one")


def test_full_size_runs_stay_on_the_fast_path():
    """trees that are runs [0, c] with the commit key c: after the load and elect_all every leader's chain is in the
    form the same chains built by AppendEntries + Heartbeat + JG_CMD_RESTART have - the dense ticks take the same
    launches and leave the same columns (the timers aside: the twin drew more)"""
    G, R = 1 << 20, 5
    rng = np.random.default_rng(2)
    c = rng.integers(0, 24, G).astype(np.uint64)
    n = (c + 1).astype(np.int64)
    off = np.zeros(G + 1, np.uint64)
    off[1:] = np.cumsum(n)
    grp = np.repeat(np.arange(G), n)
    ids = (np.arange(int(off[-1])) - off[grp].astype(np.int64)).astype(np.uint64)
    nxt = np.maximum(ids.astype(np.int64) - 1, 0).astype(np.uint64)
    dev = BatchedRaft(G, R, seed=1)
    dev.load_chains(now_ms=0, off=off, blk_id=ids, blk_next=nxt, commit=c, has_commit=np.ones(G, np.uint8))
    twin = BatchedRaft(G, R, seed=1)
    g = np.arange(G, dtype=np.uint32)
    ae = ids != 0  # AppendEntries with blocks 1 .. c, then the Heartbeat that commits c, then the restart
    first = np.zeros(G, np.uint64)
    first[1:] = np.cumsum(c)[:-1]
    twin.submit_columns(np.full(G, capi.CMD_APPEND_ENTRIES, np.uint8), g, from_=np.full(G, 2, np.uint32),
                        term=np.ones(G, np.uint64), id=first, aux=c, blk_id=ids[ae], blk_next=nxt[ae])
    twin.submit_columns(np.full(G, capi.CMD_HEARTBEAT, np.uint8), g, from_=np.full(G, 2, np.uint32),
                        term=np.ones(G, np.uint64), id=c)
    twin.step(0)
    twin.apply_all(Command.Restart(), 0)
    for e in (dev, twin):
        e.drain_messages(), e.drain_applies(), e.drain_faults()
    from josefine_amd.traces import elect_all
    skip = {"election_time", "election_timeout"}
    fields = [f for f in capi.FIELD_NAMES if f not in skip]
    compare_snapshots(dev, twin, "loaded vs restarted", fields)
    for e in (dev, twin):
        elect_all(e, 10)
        e.drain_messages(), e.drain_applies()
    compare_snapshots(dev, twin, "elected", fields)
    l0 = [e.counters()["launches"] for e in (dev, twin)]
    for t in range(4):
        acks = np.repeat(dev.read("head")[None, :], R, axis=0)  # every follower has the leader's chain
        for e in (dev, twin):
            e.step_dense_acks(acks)
    compare_snapshots(dev, twin, "dense ticks", fields)
    l1 = [e.counters()["launches"] for e in (dev, twin)]
    assert l1[0] - l0[0] == l1[1] - l0[1], (l0, l1)  # the same kernels: no slow path the twin does not take
    # (Q8: a leader elected right after Chain::new has id_gen == head and dies on its first append - on both, alike)
    assert np.array_equal(dev.read("fault"), twin.read("fault"))
    assert int(dev.read("commit").max()) > 0
