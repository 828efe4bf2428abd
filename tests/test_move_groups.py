"""jg_engine_export_groups / jg_engine_import_groups (ABI v12): live groups handed between engines without a restart.  An
engine C that imports the state image of engine A's groups continues them bit for bit: after the move, A, C and tests/ref_py
are fed the same batches and stay equal - snapshots of every field, every drained row.  Cases whose id contains "small"
are small enough for the emulated device (tests/test_move_groups_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, capi, move_groups
from josefine_amd.engine import EngineError
from fuzz import random_batch
from parity import compare_drains, compare_snapshots
from ref_py.engine import RefEngine

pytestmark = pytest.mark.gpu

DRAINS = ("drain_messages", "drain_applies", "drain_faults")


def drive(pairs, ref, rng, steps, now, rows, budget, what="", recreate=0.0, compact_at=None, foreign=True, between=None):
    """`pairs`: [(engine, clock shift)]; every engine and ref get the same batches, engine e stepped at now + shift.
    After every step each engine's drains equal ref's."""
    for s in range(steps):
        b = random_batch(rng, ref, rows, foreign_voters=foreign, budget=budget)
        now += int(rng.integers(0, 300))
        rec = np.nonzero(rng.random(ref.G) < recreate)[0]
        for e, shift in pairs + [(ref, 0)]:
            e.submit_columns(**b)
            for g in rec:
                e.submit(int(g), Command.Recreate())
            e.step((now + shift) % (1 << 64))  # (the timers are u64: they wrap)
        if s == compact_at:
            got = [e.chain_compact_resident() for e, _ in pairs + [(ref, 0)]]
            assert all(x.tobytes() == got[-1].tobytes() for x in got), what
        want = {fn: getattr(ref, fn)() for fn in DRAINS}
        for e, _ in pairs:
            for fn, w in want.items():
                got = getattr(e, fn)()
                assert got.tobytes() == w.tobytes(), (what, s, fn, len(got), len(w))
        if between is not None:
            between(s)
    return now


def engines(G, R, n, rng=None, **kw):
    return [BatchedRaft(G, R, **kw) for _ in range(n)]


def drain_all(*es):
    for e in es:
        for fn in DRAINS:
            getattr(e, fn)()


def lag_escapes(e):
    """leaders whose packed progress holds an escape (a slot far BEHIND its chain head, or ABOVE it)"""
    role, head = e.read("role"), e.read("head").astype(np.int64)
    behind = above = 0
    bits = 64 // (e.R + 1)
    for r in range(e.R):
        m = e.read("match", r).astype(np.int64)
        lead = role == capi.ROLE_LEADER
        behind += int((lead & (head - m >= (1 << bits) - 2)).sum())
        above += int((lead & (m > head)).sum())
    return behind, above


def mixed_history(G, R, flags, seed, steps=30, rows=None):
    """A and ref after a fuzzed stream with recreations and a compaction, foreign voters, then a dense ack tick on
    every group (the non-leaders take JG_FAULT_ENGINE_DENSE_NONLEADER: engine-domain faults)"""
    rng = np.random.default_rng(seed)
    kw = dict(seed=R + 3, flags=flags, self_slots=rng.integers(0, R, G).astype(np.uint8), election_timeout_ms=(300, 700))
    a, ref = BatchedRaft(G, R, **kw), RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    rows = rows or (3 * G if G < 1000 else 4000)
    now = drive([(a, 0)], ref, rng, steps, 0, rows, budget, "history", recreate=0.01, compact_at=steps // 2)
    # a few groups take a dense ack tick: the ones that do not lead fault in the engine's domain; the leaders append
    # 1100 blocks that nobody acknowledges (R = 5: every other slot's lag leaves its 10-bit field - BEHIND escapes)
    acks = np.full((R, G), capi.NO_ACK, np.uint64)
    some = rng.random(G) < 0.05
    lead = a.read("role") == capi.ROLE_LEADER
    own = kw["self_slots"].astype(np.int64)
    acks[:, some & ~lead] = a.read("head")[some & ~lead] + 1
    acks[own[some], np.nonzero(some)[0]] = np.where(lead[some], 1100, 0).astype(np.uint64)
    for e in (a, ref):
        e.step_dense_acks(acks)
    compare_drains(a, ref, "dense acks")
    compare_snapshots(a, ref, "history")
    return a, ref, kw, rng, budget, now


# ---- 1. exact continuation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R,flags", [
    pytest.param(96, 1, 0, id="small-1"),
    pytest.param(96, 3, 0, id="small-3"),
    pytest.param(96, 3, capi.CFG_SEPARATE_COMMIT_KEY, id="small-3-separate"),
    pytest.param(128, 5, capi.CFG_SEPARATE_COMMIT_KEY, id="small-5-separate"),
    pytest.param(96, 5, 0, id="small-5"),
    pytest.param(65536, 5, 0, id="65536-5"),
    pytest.param(65536, 3, capi.CFG_SEPARATE_COMMIT_KEY, id="65536-3-separate"),
])
def test_exact_continuation(G, R, flags):
    a, ref, kw, rng, budget, now = mixed_history(G, R, flags, G + 7 * R + flags, steps=30 if G < 1000 else 12)
    fault, role = a.read("fault"), a.read("role")
    if G >= 1000:  # what the image must carry
        assert (fault >= 128).any() and ((fault > 0) & (fault < 128)).any()
        assert (role == capi.ROLE_LEADER).sum() > 0 and (role == capi.ROLE_CANDIDATE).sum() > 0
        if R == 5:
            assert lag_escapes(a)[0] > 0
    # C: a fresh engine of the same node (same seed and global ids; default own slots - the image brings its own)
    c = BatchedRaft(G, R, seed=kw["seed"], flags=flags, election_timeout_ms=kw["election_timeout_ms"])
    img = a.export_groups()
    assert img.n == G and img.record_bytes % 64 == 0 and img.record_bytes == (384 if R <= 7 else 448)
    assert img.n_replicas == R and img.node_ids == a.node_ids and img.global0 == 0 and img.seed == kw["seed"]
    c.import_groups(img)
    compare_snapshots(c, a, "imported")
    assert c.export_groups().records.tobytes() == img.records.tobytes()
    drive([(a, 0), (c, 0)], ref, rng, 50 if G < 1000 else 20, now, 3 * G if G < 1000 else 4000, budget, "continued",
          recreate=0.005, between=lambda s: compare_snapshots(c, a, f"step {s}") if G < 1000 or s % 5 == 4 else None)
    compare_snapshots(c, ref, "end")
    compare_snapshots(a, ref, "end")


# ---- 2. relocation and clock ------------------------------------------------------------------------------------------
def sub_batch(b, lo, hi, to):
    """the rows of groups [lo, hi) of batch b, renumbered to start at `to`"""
    k = (b["group"] >= lo) & (b["group"] < hi)
    out = {n: (v[k] if n not in ("blk_id", "blk_next") else v) for n, v in b.items()}
    out["group"] = (out["group"] - lo + to).astype(np.uint32)
    return out


def sub_rows(rows, lo, hi, to):
    k = (rows["group"] >= lo) & (rows["group"] < hi)
    out = rows[k].copy()
    out["group"] = out["group"] - lo + to
    return out


def test_small_relocation_same_global_id():
    """A's groups [32, 64) land at C's local 8 .. 39; C's group_base is 24, so their global ids are the same: the
    continuation is exact, election timeouts included"""
    G, R = 96, 3
    a, ref, kw, rng, budget, now = mixed_history(G, R, 0, 5)
    lo, hi, to = 32, 64, 8
    c = BatchedRaft(48, R, seed=kw["seed"], group_base=lo - to, election_timeout_ms=kw["election_timeout_ms"])
    img = a.export_groups(lo, hi - lo)
    assert img.global0 == lo and img.g0 == lo
    c.import_groups(img, g0=to)
    for f in capi.FIELD_NAMES:
        for r in range(R if f == "match" else 1):
            x, y = (c.read(f, r), a.read(f, r)) if f == "match" else (c.read(f), a.read(f))
            assert np.array_equal(x[to:to + hi - lo], y[lo:hi]), f
    for s in range(50):
        b = random_batch(rng, ref, 3 * G, foreign_voters=True, budget=budget)
        now += int(rng.integers(0, 300))
        for e in (a, ref):
            e.submit_columns(**b)
            e.step(now)
        c.submit_columns(**sub_batch(b, lo, hi, to))
        c.step(now)
        for fn in DRAINS:
            w, x, y = getattr(ref, fn)(), getattr(a, fn)(), getattr(c, fn)()
            assert x.tobytes() == w.tobytes(), (s, fn)
            assert sub_rows(w, lo, hi, to).tobytes() == y.tobytes(), (s, fn)
        for f in ("term", "role", "commit", "head", "election_time", "election_timeout", "fault", "voted_for"):
            if f in capi.FIELD_NAMES:
                assert np.array_equal(c.read(f)[to:to + hi - lo], a.read(f)[lo:hi]), (s, f)


def ref_move(src, gs, dst, gd):
    """ref_py's hand-over of group gs of `src` to group gd of `dst`: the same Raft object, its draw count, its fault and
    own slot; future timeouts drawn under the destination's global id"""
    g = src.groups[gs]
    g.rand_range = dst._rand(gd)
    dst.groups[gd] = g
    dst.draws[gd] = src.draws[gs]
    dst.fault[gd] = src.fault[gs]
    dst.slots[gd] = src.slots[gs]


def test_small_relocation_other_global_id_equals_ref_py():
    """the move to another global id: exact given the destination's draws - ref_py moved the same way agrees"""
    G, R = 96, 3
    a, ref, kw, rng, budget, now = mixed_history(G, R, 0, 6)
    lo, hi, to = 16, 80, 0
    kwc = dict(seed=kw["seed"] + 1, group_base=1000, election_timeout_ms=kw["election_timeout_ms"])
    c, rc = BatchedRaft(hi - lo, R, **kwc), RefEngine(hi - lo, R, **kwc)
    move_groups(a, c, lo, hi - lo, dst_g0=to)
    for i in range(hi - lo):
        ref_move(ref, lo + i, rc, to + i)
    compare_snapshots(c, rc, "moved")
    budget_c = np.full(hi - lo, 1)  # (the moved chains keep their segments; few new forks)
    drive([(c, 0)], rc, rng, 50, now, 3 * (hi - lo), budget_c, "other global id")
    compare_snapshots(c, rc, "end")


@pytest.mark.parametrize("shift", [pytest.param(7_000_000, id="small-plus"), pytest.param(-123_456, id="small-minus")])
def test_small_clock_shift(shift):
    """imported with shift_ms, C driven at now + shift equals A driven at now (wrapping u64 arithmetic)"""
    G, R = 96, 3
    a, ref, kw, rng, budget, now = mixed_history(G, R, capi.CFG_SEPARATE_COMMIT_KEY, 8)
    c = BatchedRaft(G, R, seed=kw["seed"], flags=capi.CFG_SEPARATE_COMMIT_KEY, election_timeout_ms=kw["election_timeout_ms"])
    c.import_groups(a.export_groups(), shift_ms=shift)
    et = a.read("election_time").astype(np.uint64)
    assert np.array_equal(c.read("election_time"), et + np.uint64(shift % (1 << 64)))
    drive([(a, 0), (c, shift)], ref, rng, 50, now, 3 * G, budget, "shift",
          between=lambda s: compare_snapshots(c, a, f"step {s}", fields=[f for f in capi.FIELD_NAMES if f not in ("election_time", "heartbeat_time")]))


# ---- 3. round trip and side effects -----------------------------------------------------------------------------------
def test_small_export_has_no_side_effects():
    G, R = 64, 3
    rng = np.random.default_rng(3)
    kw = dict(seed=6, self_slots=rng.integers(0, R, G).astype(np.uint8), election_timeout_ms=(300, 700))
    a, b, ref = BatchedRaft(G, R, **kw), BatchedRaft(G, R, **kw), RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    images = []

    def between(s):
        images.append(a.export_groups())
        if s % 3 == 0:
            images.append(a.export_groups(5, 17))
        compare_snapshots(a, b, f"step {s}")

    drive([(a, 0), (b, 0)], ref, rng, 40, 0, 3 * G, budget, "exports", recreate=0.01, compact_at=20, between=between)
    compare_snapshots(a, ref, "end")
    assert images[0].records.tobytes() != images[-1].records.tobytes()
    # round trip: export(import(export(A))) == export(A)
    c = BatchedRaft(G, R, seed=6)
    img = a.export_groups()
    c.import_groups(img)
    assert c.export_groups().records.tobytes() == img.records.tobytes()
    sub = a.export_groups(5, 17)
    assert sub.records.tobytes() == img.records[5:22].tobytes() and sub.global0 == 5


# ---- 4. paths ---------------------------------------------------------------------------------------------------------
def test_small_node_steps_and_dense_ticks():
    """imports between node steps (plain and JG_NODE_ASYNC; refused while two are kept); dense ack ticks continue on
    imported FAST leaders, and non-FAST imported leaders take k_dense_slow: equal to the twin"""
    from josefine_amd.traces import elect_all
    G, R = 256, 3
    a, t = BatchedRaft(G, R, seed=2), BatchedRaft(G, R, seed=2)
    for e in (a, t):
        elect_all(e, 10)
        drain_all(e)
    for k in range(3):
        acks = np.repeat(a.read("head")[None, :] + 1, R, axis=0)
        acks[0] = 1
        for e in (a, t):
            e.step_dense_acks(acks)
    # some leaders leave FAST form: restarted (id_gen = commit = head, Q8) and elected again
    from node_step import elect_some
    for e in (a, t):
        for g in range(0, G, 7):
            e.submit(g, Command.Restart())
        e.step(500)
        elect_some(e, np.arange(G) % 7 == 0, now_ms=550)
        e.submit_columns(kind=np.full(G // 2, capi.CMD_TIMEOUT, np.uint8), group=np.arange(1, G, 2, dtype=np.uint32))
        e.step(600)
    drain_all(a, t)
    c = BatchedRaft(G, R, seed=2)
    img = a.export_groups()
    # the premise, read from the image's flag words (record word 8): healthy leaders in FAST form and out of it
    f = img.records.view(np.uint64).reshape(G, -1)[:, 8].astype(np.int64)
    leader, healthy, fast = (f & 3) == capi.ROLE_LEADER, ((f >> 16) & 0xFF) == 0, (f & 0x10) != 0
    assert (leader & healthy & ~fast).sum() >= 8 and (leader & healthy & fast).sum() >= 64
    c.import_groups(img)
    compare_snapshots(c, t, "imported")
    for k in range(4):
        acks = np.repeat(t.read("head")[None, :] + 1, R, axis=0)
        acks[0] = 1
        acks[1, ::5] = capi.NO_ACK
        for e in (c, t):
            e.step_dense_acks(acks)
        compare_drains(c, t, f"dense {k}")
        compare_snapshots(c, t, f"dense {k}")
    for r in range(3):
        for e in (c, t):
            e.step_node(2000 + 50 * r)
        compare_drains(c, t, f"node {r}")
        compare_snapshots(c, t, f"node {r}")
    # an async node step is settled by the export; the import goes between node steps
    for e in (c, t):
        e.step_node_begin(3000, async_=True)
    img = c.export_groups()
    for e in (c, t):
        e.node_outbox()
    d = BatchedRaft(G, R, seed=2)
    d.step_node(3000)  # (a node step before the import)
    drain_all(d)
    d.import_groups(img)
    compare_snapshots(d, t, "async")
    # two kept steps outstanding: both calls refuse, nothing changes
    d.step_node_begin(3100, async_=True, keep=True)
    d.step_node_begin(3150, async_=True, keep=True)
    with pytest.raises(EngineError):
        d.export_groups()
    with pytest.raises(EngineError):
        d.import_groups(img)
    d.node_outbox(), d.node_outbox()
    t.step_node(3100), t.step_node(3150)
    drain_all(d, t)
    compare_snapshots(d, t, "kept")


@pytest.mark.parametrize("R", [3])
def test_routed_cluster_node_imported_between_rounds(R):
    """one node of a jg_dense_cluster (JG_CLUSTER_ANY_LEADER) handed over between routed rounds: its groups are exported,
    overwritten by the image of a fresh engine (so that nothing of them is left in place), and imported back from the
    image; the rounds go on exactly as an untouched cluster's"""
    from josefine_amd import DenseCluster as LibCluster
    from test_any_leader import spread_leaders
    G = 1200
    clusters = []
    for _ in range(2):
        nodes = [BatchedRaft(G, R, seed=5 + r, self_slots=np.full(G, r, np.uint8)) for r in range(R)]
        spread_leaders(nodes, G, R)
        lib = LibCluster(nodes, lead=None)
        lib.set_appends(1)
        clusters.append((nodes, lib))
    for t in range(12):
        for nodes, lib in clusters:
            lib.round_routed((t + 1) * 100)
        if t % 4 == 1:
            nodes = clusters[0][0]
            for n in range(R):
                img = nodes[n].export_groups()
                nodes[n].import_groups(BatchedRaft(G, R, seed=5 + n, self_slots=np.full(G, n, np.uint8)).export_groups())
                assert not np.array_equal(nodes[n].read("term"), clusters[1][0][n].read("term"))
                assert nodes[n].export_groups().records.tobytes() != img.records.tobytes()
                nodes[n].import_groups(img)
        for n in range(R):
            compare_snapshots(clusters[0][0][n], clusters[1][0][n], f"round {t} node {n}")
    assert int(clusters[0][0][0].read("commit").min()) > 0
    for _, lib in clusters:
        lib.close()


def test_small_device_form():
    G, R = 200, 5
    a, ref, kw, rng, budget, now = mixed_history(G, R, 0, 12)
    img = a.export_groups(device=True)
    host = a.export_groups()
    assert img.to_host().tobytes() == host.records.tobytes()
    c = BatchedRaft(G, R, seed=kw["seed"], election_timeout_ms=kw["election_timeout_ms"])
    c.import_groups(img)
    compare_snapshots(c, a, "device form")
    img.free()
    drive([(a, 0), (c, 0)], ref, rng, 10, now, 3 * G, budget, "device form")


# ---- 5. refusals leave the destination unchanged ----------------------------------------------------------------------
def raw_import(e, img, g0=0, records=None, **hdr):
    x = capi.GroupImport()
    x.g0 = g0
    x.header = img.header
    for k, v in hdr.items():
        if k == "node_ids":
            for r, nid in enumerate(v):
                x.header.node_ids[r] = nid
        else:
            setattr(x.header, k, v)
    rec = np.ascontiguousarray(img.records if records is None else records)
    x.records = rec.ctypes.data
    return e.api.engine_import_groups(e._h, C.byref(x))


def check_word(rec):
    """the check word of one record (jg_move.h): every word but word 0 hashed with its index, XOR-folded"""
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9e3779b97f4a7c15) & M
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M
        return z ^ (z >> 31)
    w = rec.view(np.uint64)
    c = mix(0x6a6f73656d6f7665 ^ len(w))
    for k in range(1, len(w)):
        c ^= mix(int(w[k]) ^ ((k * 0x9e3779b97f4a7c15) & M))
    return c


def test_small_refusals():
    G, R = 1000, 3
    src = BatchedRaft(G, R, seed=4)
    from josefine_amd.traces import elect_all
    elect_all(src, 10)
    img = src.export_groups()
    assert all(check_word(img.records[i]) == int(img.records[i].view(np.uint64)[0]) for i in range(0, G, 97))
    dst, twin = BatchedRaft(G, R, seed=4), BatchedRaft(G, R, seed=4)  # (the twin gets every call but the refused ones)
    for e in (dst, twin):
        e.step(5)
    before = dst.export_groups().records.tobytes()

    def unchanged(rc, what):
        assert rc == capi.EINVAL, (what, rc)
        assert dst.export_groups().records.tobytes() == before, what

    unchanged(raw_import(dst, img, g0=1), "range")
    unchanged(raw_import(dst, img, format=2), "format")
    unchanged(raw_import(dst, img, record_bytes=448), "record_bytes")
    unchanged(raw_import(dst, img, n_replicas=2), "R")
    unchanged(raw_import(dst, img, node_ids=[1, 2, 9]), "node_ids")
    unchanged(raw_import(dst, img, separate_commit_key=1), "commit key")
    other = BatchedRaft(G, 5, seed=4)
    with pytest.raises(EngineError):
        other.import_groups(img)
    # one byte flipped in one record of a 1 000-record image
    bad = img.records.copy()
    bad[613, 77] ^= 0x10
    unchanged(raw_import(dst, img, records=bad), "flipped byte")
    # an own slot >= R with a recomputed check word
    bad = img.records.copy()
    w = bad[500].view(np.uint64)
    w[8] = (int(w[8]) & ~(0x7 << 24)) | (R << 24)
    w[0] = check_word(bad[500])
    unchanged(raw_import(dst, img, records=bad), "own slot")
    # a window count above JG_CHAIN_WINDOW and a role out of range, check words recomputed
    for mask, val in ((0xF << 28, 9 << 28), (0x3, 3)):
        bad = img.records.copy()
        w = bad[7].view(np.uint64)
        w[8] = (int(w[8]) & ~mask) | val
        w[0] = check_word(bad[7])
        unchanged(raw_import(dst, img, records=bad), "range of a field")
    # queued commands: refused, the queued rows still there and applied by the next step, as on the twin
    for e in (dst, twin):
        e.submit_columns(kind=np.full(G, capi.CMD_TIMEOUT, np.uint8), group=np.arange(G, dtype=np.uint32))
    assert dst.export_groups().records.tobytes() == before
    with pytest.raises(EngineError):
        dst.import_groups(img)
    assert dst.export_groups().records.tobytes() == before
    for e in (dst, twin):
        e.step(6)
    compare_drains(dst, twin, "queued")
    compare_snapshots(dst, twin, "queued")
    assert dst.export_groups().records.tobytes() == twin.export_groups().records.tobytes() != before
    # kept node steps: refused, and both steps deliver as the twin's
    outs = []
    for e in (dst, twin):
        e.step_node_begin(800, async_=True, keep=True)
        e.step_node_begin(900, async_=True, keep=True)
    assert raw_import(dst, img) == capi.EINVAL
    for e in (dst, twin):
        outs.append([e.node_outbox(), e.node_outbox()])
    for k in range(2):
        for name in outs[0][k]:
            assert np.array_equal(np.asarray(outs[0][k][name]), np.asarray(outs[1][k][name])), ("kept", k, name)
    compare_drains(dst, twin, "kept")
    compare_snapshots(dst, twin, "kept")
    assert dst.export_groups().records.tobytes() == twin.export_groups().records.tobytes()
    # the device form on a multi-device handle
    s = BatchedRaft(G, R, seed=4, device_ids=[0, 0])
    x = capi.GroupExport()
    x.n, x.flags, x.cap_bytes = G, capi.MOVE_DEVICE, G * img.record_bytes
    x.records = 256
    assert s.api.engine_export_groups(s._h, C.byref(x)) == capi.EINVAL
    xi = capi.GroupImport()
    xi.header, xi.flags, xi.records = img.header, capi.MOVE_DEVICE, 256
    assert s.api.engine_import_groups(s._h, C.byref(xi)) == capi.EINVAL
    # the sizing call: the header, JG_ECAPACITY, nothing written
    x = capi.GroupExport()
    x.g0, x.n = 3, 10
    assert src.api.engine_export_groups(src._h, C.byref(x)) == capi.ECAPACITY
    assert x.header.n == 10 and x.header.record_bytes == 384 and x.header.global0 == 3
    # a valid import still works after all of this
    dst.import_groups(img)
    compare_snapshots(dst, src, "after the refusals")


# ---- 6. full size and shards (GPU only) -------------------------------------------------------------------------------
def test_full_size_and_shards():
    from josefine_amd.traces import elect_all
    G, R = 1 << 20, 5
    a = BatchedRaft(G, R, seed=3)
    elect_all(a, 10)
    rng = np.random.default_rng(1)
    for k in range(3):
        acks = np.repeat(a.read("head")[None, :] + 1, R, axis=0)
        acks[0] = 1
        acks[2, rng.random(G) < 0.1] = capi.NO_ACK
        a.step_dense_acks(acks)
    a.submit_columns(kind=np.full(G // 64, capi.CMD_TIMEOUT, np.uint8), group=np.arange(0, G, 64, dtype=np.uint32))
    a.step(900)
    drain_all(a)
    img = a.export_groups()
    c = BatchedRaft(G, R, seed=3)
    c.import_groups(img)
    compare_snapshots(c, a, "1M")
    assert c.export_groups().records.tobytes() == img.records.tobytes()
    acks = np.repeat(a.read("head")[None, :] + 1, R, axis=0)
    acks[0] = 1
    c.step_dense_acks(acks)  # (the twin of every sharded handle's tick below)
    for D in (2, 3):
        s = BatchedRaft(G, R, seed=3, device_ids=[0] * D)
        s.import_groups(img)
        compare_snapshots(s, a, f"{D} shards")
        assert s.export_groups().records.tobytes() == img.records.tobytes()
        g0, n = G // 3 - 5, G // 2
        assert s.export_groups(g0, n).records.tobytes() == img.records[g0:g0 + n].tobytes()
        s.step_dense_acks(acks)
        compare_snapshots(s, c, f"{D} shards, a tick on")
        del s
