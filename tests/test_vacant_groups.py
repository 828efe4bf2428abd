"""Vacant slots (ABI v13): jg_engine_open_groups / jg_engine_close_groups / jg_engine_list_groups and JG_CFG_START_VACANT.
A closed slot hosts no partition: it ignores every row (JG_CMD_RESTART / JG_CMD_RECREATE included), emits nothing under
jg_step or jg_step_node, and holds the canonical vacant record; the hosted slots of the same engine go on exactly as on a
control engine and tests/ref_py.  Opening a slot is what a JG_CMD_RECREATE row does.  Cases whose id contains "small" are
small enough for the emulated device (tests/test_vacant_groups_emulated.py)."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, capi, move_groups
from josefine_amd.engine import EngineError
from fuzz import random_batch
from parity import compare_drains, compare_snapshots
from ref_py.engine import RefEngine
from test_move_groups import drain_all, drive

pytestmark = pytest.mark.gpu

VAC = capi.FAULT_VACANT
DRAINS = ("drain_messages", "drain_applies", "drain_faults")
LIST_TILE = 256 * 16  # slots per workgroup of the list passes (jg_hosting.h JG_LIST_TILE)


def records(e, g0=0, n=None):
    n = e.G - g0 if n is None else n
    return e.export_groups(g0, n).records.view(np.uint64).reshape(n, -1)


def assert_canonical(e, gs, what=""):
    """the closed slots `gs` hold the canonical vacant record: only the own slot and the draw count vary"""
    w = records(e)[gs]
    own = e.read("self_slot")[gs].astype(np.uint64)
    assert (w[:, 1:8] == np.array([0, 0, 0, 1, 0, 0, 0], np.uint64)).all(), what  # term commit head id_gen run_hi mlag hb
    assert (w[:, 8] == ((VAC << 16) | 0x80 | 0x10 | (own << 24))).all(), what  # follower, RUN + FAST, vacant, own slot
    assert (w[:, 9] == 0).all() and ((w[:, 10] & 0xFFFFFFFF) == 0).all(), what  # election time and timeout 0
    assert (w[:, 11:] == 0).all(), what
    assert (e.read("fault")[gs] == VAC).all(), what
    return w


def compare_hosted(a, b, hosted, what=""):
    for name in capi.FIELD_NAMES:
        for r in (range(a.R) if name == "match" else [0]):
            x, y = a.read(name, r)[hosted], b.read(name, r)[hosted]
            if not np.array_equal(x, y):
                bad = np.nonzero(x != y)[0][:8]
                raise AssertionError(f"{what}: {name}[{r}] differs at slots {np.asarray(hosted)[bad]}: {x[bad]} vs {y[bad]}")


def drains_without(e, want, closed, what=""):
    """e's drains equal `want` ({drain: rows}) without the rows of the closed slots - and name no closed slot"""
    for fn, w in want.items():
        got = getattr(e, fn)()
        keep = w[~np.isin(w["group"], closed)]
        assert got.tobytes() == keep.tobytes(), (what, fn, len(got), len(keep))
        assert not np.isin(got["group"], closed).any(), (what, fn)


def restart_rows(rng, gs, now_kinds=(capi.CMD_RESTART, capi.CMD_RECREATE)):
    g = np.sort(rng.choice(gs, min(len(gs), 8), replace=False)).astype(np.uint32)
    return dict(kind=rng.choice(now_kinds, len(g)).astype(np.uint8), group=g)


def fresh(G, R, seed, slots, **kw):
    base = dict(seed=seed, self_slots=slots, election_timeout_ms=(300, 700))
    base.update(kw)
    return BatchedRaft(G, R, **base), base


# ---- 1. a closed slot is inert ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,R", [pytest.param(192, 3, id="small-3"), pytest.param(160, 5, id="small-5")])
def test_close_is_inert(G, R):
    rng = np.random.default_rng(G + R)
    slots = rng.integers(0, R, G).astype(np.uint8)
    a, kw = fresh(G, R, R + 1, slots)
    b, _ = fresh(G, R, R + 1, slots)
    ref = RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    now = drive([(a, 0), (b, 0)], ref, rng, 12, 0, 3 * G, budget, "history", recreate=0.01)
    closed = np.sort(rng.choice(G, G // 3, replace=False)).astype(np.uint32)
    hosted = np.setdiff1d(np.arange(G), closed)
    a.close_groups(closed)
    vac = assert_canonical(a, closed, "closed")
    assert np.array_equal(a.vacant_groups(), closed) and np.array_equal(a.hosted_groups(), hosted)
    compare_hosted(a, b, hosted, "after the close")
    assert len(a.drain_faults()) == 0
    for s in range(25):
        batch = random_batch(rng, ref, 3 * G, foreign_voters=True, budget=budget)
        extra = restart_rows(rng, closed)
        now += int(rng.integers(0, 300))
        for e in (a, b, ref):
            e.submit_columns(**batch)
            e.submit_columns(**extra)  # (RESTART / RECREATE rows for closed slots: they must not revive them)
            e.step(now)
        want = {fn: getattr(ref, fn)() for fn in DRAINS}
        for fn, w in want.items():
            assert getattr(b, fn)().tobytes() == w.tobytes(), (s, fn)
        drains_without(a, want, closed, f"step {s}")
        compare_hosted(a, ref, hosted, f"step {s}")
        assert np.array_equal(records(a)[closed], vac), s
    compare_snapshots(b, ref, "control")
    # the node step: answers and every outbox column of a closed slot are what an all-vacant engine writes
    v, _ = fresh(G, R, R + 1, slots, start_vacant=True)
    for s in range(12):
        now += int(rng.integers(100, 400))
        batch = random_batch(rng, b, G, foreign_voters=True, budget=budget)
        extra = restart_rows(rng, closed)
        outs = []
        for e in (a, b, v):
            e.submit_columns(**batch)
            e.submit_columns(**extra)
            outs.append(e.step_node(now))
        for name, x in outs[0].items():
            if not isinstance(x, np.ndarray):
                continue
            y, z = outs[1][name], outs[2][name]
            assert np.array_equal(x[..., hosted], y[..., hosted]), (s, name)
            assert np.array_equal(x[..., closed], z[..., closed]), (s, name)
        want = {fn: getattr(b, fn)() for fn in DRAINS}
        drains_without(a, want, closed, f"node step {s}")
        for fn in DRAINS:
            assert len(getattr(v, fn)()) == 0, (s, fn)
        compare_hosted(a, b, hosted, f"node step {s}")
        assert np.array_equal(records(a)[closed], vac), s
    assert now > 5000  # (well past every election timeout)


# ---- 2. open = JG_CMD_RECREATE ----------------------------------------------------------------------------------------
def test_small_open_equals_recreate():
    G, R = 160, 3
    rng = np.random.default_rng(5)
    slots = rng.integers(0, R, G).astype(np.uint8)
    a, kw = fresh(G, R, 9, slots)
    b, _ = fresh(G, R, 9, slots)
    ref = RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    now = drive([(a, 0), (b, 0)], ref, rng, 15, 0, 3 * G, budget, "history")
    gs = np.sort(rng.choice(G, 40, replace=False))
    now += 50
    a.close_groups(gs)
    a.open_groups(gs[::-1].tolist(), now)  # (any order: sorted by the binding)
    for e in (b, ref):
        for g in gs:
            e.submit(int(g), Command.Recreate())
        e.step(now)
    drain_all(a, b, ref)
    compare_snapshots(a, b, "open vs recreate")
    compare_snapshots(a, ref, "open vs ref_py")
    ra, rb = a.read_chains(), b.read_chains()
    for k in ra:
        assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k
    drive([(a, 0), (b, 0)], ref, rng, 30, now, 3 * G, budget, "after the open")
    compare_snapshots(a, b, "continued")


def test_small_reopen_after_a_long_vacancy():
    G, R = 128, 3
    rng = np.random.default_rng(8)
    slots = rng.integers(0, R, G).astype(np.uint8)
    a, kw = fresh(G, R, 4, slots)
    ref = RefEngine(G, R, **kw)
    budget = np.full(G, capi.CHAIN_WINDOW - 2)
    now = drive([(a, 0)], ref, rng, 10, 0, 3 * G, budget, "history")
    gs = np.sort(rng.choice(G, 30, replace=False))
    hosted = np.setdiff1d(np.arange(G), gs)
    a.close_groups(gs)
    draws = records(a)[gs, 10] >> 32  # the carried draw counts
    for s in range(20):  # ref_py's copies of the closed slots go on; a's are vacant
        batch = random_batch(rng, ref, 3 * G, foreign_voters=True, budget=budget)
        now += int(rng.integers(0, 300))
        for e in (a, ref):
            e.submit_columns(**batch)
            e.step(now)
        want = {fn: getattr(ref, fn)() for fn in DRAINS}
        drains_without(a, want, gs, f"vacant {s}")
        compare_hosted(a, ref, hosted, f"vacant {s}")
    assert (records(a)[gs, 10] >> 32 == draws).all()
    now += 1000
    a.open_groups(gs, now)
    for g, d in zip(gs, draws):
        ref.draws[int(g)] = int(d)  # ref_py's recreate with the carried draw count
        ref.submit(int(g), Command.Recreate())
    ref.step(now)
    drain_all(ref)
    budget[gs] = capi.CHAIN_WINDOW - 2
    compare_snapshots(a, ref, "reopened")
    drive([(a, 0)], ref, rng, 25, now, 3 * G, budget, "after the reopen")


def test_small_open_with_self_slots():
    """an engine started vacant and opened at 0 with own slots = a fresh engine with those own slots"""
    G, R = 96, 5
    rng = np.random.default_rng(2)
    slots = rng.integers(0, R, G).astype(np.uint8)
    v = BatchedRaft(G, R, seed=6, start_vacant=True, election_timeout_ms=(300, 700))
    assert (v.read("self_slot") == 0).all()
    v.open_groups(np.arange(G), 0, self_slots=slots)
    a, kw = fresh(G, R, 6, slots)
    compare_snapshots(v, a, "opened with own slots")
    ref = RefEngine(G, R, **kw)
    drive([(v, 0), (a, 0)], ref, rng, 20, 0, 3 * G, np.full(G, capi.CHAIN_WINDOW - 2), "continued")
    # through device memory, a part of the slots with other own slots
    gs = np.arange(10, 50, 3)
    v.close_groups(gs, device=True)
    assert_canonical(v, gs, "device close")
    new = (v.read("self_slot")[gs] + 1) % R
    v.open_groups(gs, 9000, self_slots=new, device=True)
    assert np.array_equal(v.read("self_slot")[gs], new) and not (v.read("fault")[gs] == VAC).any()


# ---- 3. JG_CFG_START_VACANT -------------------------------------------------------------------------------------------
def test_small_start_vacant():
    G, R = 128, 3
    rng = np.random.default_rng(3)
    v = BatchedRaft(G, R, seed=1, start_vacant=True)
    ref = RefEngine(G, R, seed=1)
    assert (v.read("fault") == VAC).all()
    assert np.array_equal(v.vacant_groups(), np.arange(G)) and v.hosted_groups().size == 0
    assert v.count_groups() == G and v.count_groups(vacant=False) == 0
    rec = records(v)
    for s in range(6):
        batch = random_batch(rng, ref, 3 * G, foreign_voters=True)
        for e in (v, ref):
            e.submit_columns(**batch)
            e.submit_columns(kind=np.full(G, capi.CMD_RECREATE, np.uint8), group=np.arange(G, dtype=np.uint32))
            e.step(1000 * (s + 1))
        drain_all(ref)
        for fn in DRAINS:
            assert len(getattr(v, fn)()) == 0, (s, fn)
        out = v.step_node(1000 * s + 500)
        assert (out["answer"] == capi.NO_ACK).all(), s
        for fn in DRAINS:
            assert len(getattr(v, fn)()) == 0, (s, fn)
    assert np.array_equal(records(v), rec)
    assert len(v.read_trees()) == G and all(t is None for t in v.read_trees())


def test_small_start_vacant_opens_elect_exactly_those():
    G, R = 96, 1
    v = BatchedRaft(G, R, seed=2, start_vacant=True)
    gs = np.array([0, 5, 6, 40, 63, 64, 95])
    v.open_groups(gs, 0)
    for t in range(1, 6):
        v.step_node(1100 * t)
    drain_all(v)
    role = v.read("role")
    assert np.array_equal(np.nonzero(role == capi.ROLE_LEADER)[0], gs)
    assert np.array_equal(v.hosted_groups(), gs)
    assert (v.read("term")[gs] >= 1).all() and (v.read("term")[np.setdiff1d(np.arange(G), gs)] == 0).all()


def test_small_load_chains_opens_a_vacant_range():
    G, R = 64, 3
    v = BatchedRaft(G, R, seed=3, start_vacant=True)
    trees = [([(0, 0)] + [(i, i - 1) for i in range(1, k + 2)], k) for k in range(10)]
    v.load_chains(trees, now_ms=100, g0=20)
    want = np.setdiff1d(np.arange(G), np.arange(20, 30))
    assert np.array_equal(v.vacant_groups(), want)
    assert (v.read("fault")[20:30] == 0).all() and np.array_equal(v.read("commit")[20:30], np.arange(10))
    assert [t[1] for t in v.read_trees(20, 10)] == list(range(10))


# ---- 4. list_groups --------------------------------------------------------------------------------------------------
def check_lists(e, what=""):
    vac = e.read("fault") == VAC
    G = e.G
    cuts = [(0, G), (1, G - 1), (LIST_TILE - 3, 7), (LIST_TILE, LIST_TILE + 1), (G - 5, 5), (0, 0), (G // 3, G // 2)]
    for g0, n in cuts:
        if g0 < 0 or g0 + n > G:
            continue
        for which, mask in ((e.vacant_groups, vac), (e.hosted_groups, ~vac)):
            want = (g0 + np.nonzero(mask[g0:g0 + n])[0]).astype(np.uint32)
            assert np.array_equal(which(g0, n), want), (what, g0, n)
            for lim in (0, 1, len(want) - 1, len(want), len(want) + 5):
                if lim >= 0:
                    got = which(g0, n, limit=lim)
                    assert got.dtype == np.uint32 and np.array_equal(got, want[:lim]), (what, g0, n, lim)
        assert e.count_groups(True, g0, n) == int(vac[g0:g0 + n].sum()), (what, g0, n)


def test_small_list_groups():
    G, R = 3 * LIST_TILE + 77, 1
    rng = np.random.default_rng(4)
    e = BatchedRaft(G, R, seed=5)
    check_lists(e, "all hosted")
    edges = [0, 1, 63, 64, 255, 256, LIST_TILE - 1, LIST_TILE, 2 * LIST_TILE - 1, 2 * LIST_TILE, G - 1]
    rand = rng.choice(G, G // 3, replace=False)
    e.close_groups(np.union1d(edges, rand))
    check_lists(e, "random")
    e.open_groups(e.vacant_groups(LIST_TILE, LIST_TILE))  # (a whole tile hosted again)
    e.close_groups(range(LIST_TILE + 10, LIST_TILE + 300))
    check_lists(e, "mixed")
    e.open_groups(e.vacant_groups())
    assert e.count_groups() == 0
    e.close_groups(range(G))
    check_lists(e, "all vacant")
    with pytest.raises(EngineError):
        e.vacant_groups(G - 1, 2)


def test_list_groups_16m():
    G = 1 << 24
    rng = np.random.default_rng(6)
    e = BatchedRaft(G, 1, seed=1, start_vacant=True)
    assert e.count_groups() == G
    gs = np.unique(rng.integers(0, G, 5_000_000)).astype(np.uint32)
    e.open_groups(gs)
    vac = e.read("fault") == VAC
    assert not vac[gs].any() and int(vac.sum()) == G - gs.size
    assert np.array_equal(e.hosted_groups(), gs)
    assert np.array_equal(e.vacant_groups(), np.nonzero(vac)[0].astype(np.uint32))
    assert np.array_equal(e.vacant_groups(limit=1000), np.nonzero(vac)[0][:1000])
    assert np.array_equal(e.hosted_groups(G // 2, G // 4), gs[(gs >= G // 2) & (gs < G // 2 + G // 4)])


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def raw(e, fn, groups=None, g0=0, n=0, self_slots=None, now=0):
    s = capi.GroupSet()
    keep = []
    if groups is not None:
        lst = np.ascontiguousarray(groups, dtype=np.uint32)
        keep.append(lst)
        s.groups, s.n = lst.ctypes.data, lst.size
    else:
        s.g0, s.n = g0, n
    if self_slots is not None:
        own = np.ascontiguousarray(self_slots, dtype=np.uint8)
        keep.append(own)
        s.self_slots = own.ctypes.data
    if fn == "open":
        return e.api.engine_open_groups(e._h, now, C.byref(s))
    return e.api.engine_close_groups(e._h, C.byref(s))


def test_small_refusals():
    G, R = 300, 3
    from josefine_amd.traces import elect_all
    e, twin = BatchedRaft(G, R, seed=4), BatchedRaft(G, R, seed=4)
    for x in (e, twin):
        elect_all(x, 10)
        x.close_groups(range(100, 200))
        drain_all(x)
    before = records(e).tobytes()

    def unchanged(rc, what):
        assert rc == capi.EINVAL, (what, rc)
        assert records(e).tobytes() == before, what

    unchanged(raw(e, "close", [5, G]), "index out of range")
    unchanged(raw(e, "close", g0=250, n=51), "range out of bounds")
    unchanged(raw(e, "open", [150, 120]), "descending")
    unchanged(raw(e, "open", [120, 120]), "duplicate")
    unchanged(raw(e, "close", [1, 2, 3, 3]), "duplicate")
    unchanged(raw(e, "open", [150, 151, 5]), "open a hosted slot")
    unchanged(raw(e, "open", g0=190, n=20), "open a hosted range")
    unchanged(raw(e, "close", [5, 6, 150]), "close a vacant slot")
    unchanged(raw(e, "open", [150, 160], self_slots=[0, R]), "own slot >= R")
    with pytest.raises(EngineError):
        e.open_groups([150, 160, 150])  # (the binding refuses a duplicate itself)
    # queued commands: refused, the rows stay queued and are applied by the next step as on the twin
    for x in (e, twin):
        x.submit_columns(kind=np.full(G, capi.CMD_TIMEOUT, np.uint8), group=np.arange(G, dtype=np.uint32))
    assert raw(e, "open", [150]) == capi.EINVAL and raw(e, "close", [5]) == capi.EINVAL
    for x in (e, twin):
        x.step(900)
    compare_drains(e, twin, "queued")
    compare_snapshots(e, twin, "queued")
    # kept node steps: refused, both steps deliver as the twin's
    for x in (e, twin):
        x.step_node_begin(1000, async_=True, keep=True)
        x.step_node_begin(1100, async_=True, keep=True)
    assert raw(e, "open", [150]) == capi.EINVAL and raw(e, "close", [5]) == capi.EINVAL
    outs = [[x.node_outbox(), x.node_outbox()] for x in (e, twin)]
    for k in range(2):
        for name, v in outs[0][k].items():
            assert np.array_equal(np.asarray(v), np.asarray(outs[1][k][name])), (k, name)
    compare_drains(e, twin, "kept")
    compare_snapshots(e, twin, "kept")
    # the device form on a multi-device handle
    s = BatchedRaft(G, R, seed=4, device_ids=[0, 0])
    gs = capi.GroupSet()
    gs.n, gs.groups, gs.flags = 1, 256, capi.GROUPS_DEVICE
    assert s.api.engine_close_groups(s._h, C.byref(gs)) == capi.EINVAL
    # and valid calls still work
    e.open_groups([150, 160], 2000)
    assert (e.read("fault")[[150, 160]] == 0).all()


# ---- 6. a move completed by a close ----------------------------------------------------------------------------------
def test_small_move_completed_by_close():
    from josefine_amd.traces import elect_all
    from node_step import elect_some
    G, R = 256, 3
    src, twin = BatchedRaft(G, R, seed=2), BatchedRaft(G, R, seed=2)
    for e in (src, twin):
        elect_some(e, np.arange(G) < 128, now_ms=10)  # slots 0 .. 127 lead, 128 .. 255 follow
        drain_all(e)
    dst = BatchedRaft(G, R, seed=2)
    dst.close_groups(range(G))
    moved = [(40, 30), (150, 40)]  # a leader range and a follower range
    for g0, n in moved:
        move_groups(src, dst, g0, n, close_source=True)
    gone = np.concatenate([np.arange(g0, g0 + n) for g0, n in moved])
    stay = np.setdiff1d(np.arange(G), gone)
    assert np.array_equal(src.vacant_groups(), gone) and np.array_equal(dst.hosted_groups(), gone)
    assert_canonical(src, gone, "source")
    compare_hosted(dst, twin, gone, "moved")
    v = BatchedRaft(G, R, seed=2, start_vacant=True)  # what a vacant slot writes into the outbox
    for t in range(8):  # far past every election timeout
        now = 1500 + 700 * t
        outs = [e.step_node(now) for e in (src, dst, twin, v)]
        for name, x in outs[0].items():
            if isinstance(x, np.ndarray):
                assert np.array_equal(x[..., stay], outs[2][name][..., stay]), (t, name)
                assert np.array_equal(x[..., gone], outs[3][name][..., gone]), (t, name)
                assert np.array_equal(outs[1][name][..., gone], outs[2][name][..., gone]), (t, name)
        want = {fn: getattr(twin, fn)() for fn in DRAINS}
        drains_without(src, want, gone, f"source {t}")
        for fn, w in want.items():
            got = getattr(dst, fn)()
            assert got.tobytes() == w[np.isin(w["group"], gone)].tobytes(), (t, fn)
        compare_hosted(src, twin, stay, f"source {t}")
        compare_hosted(dst, twin, gone, f"destination {t}")
        assert_canonical(src, gone, f"source {t}")
    assert (twin.read("role")[gone[gone < 128]] == capi.ROLE_LEADER).all()
    # a vacant record imported makes the destination slot vacant
    img = src.export_groups(40, 30)
    f = BatchedRaft(G, R, seed=2)
    f.import_groups(img)
    assert np.array_equal(f.vacant_groups(), np.arange(40, 70))
    assert records(f, 40, 30).tobytes() == img.records.tobytes()


# ---- 7. scale and shards ---------------------------------------------------------------------------------------------
def test_scale_1m():
    G, R = 1 << 20, 3
    rng = np.random.default_rng(7)
    e = BatchedRaft(G, R, seed=3)
    e.close_groups(range(G // 4, G // 2))
    assert e.count_groups() == G // 4
    gs = np.unique(rng.integers(0, G, 300_000))
    hosted = gs[(gs < G // 4) | (gs >= G // 2)]
    e.close_groups(hosted)
    vac = e.read("fault") == VAC
    assert np.array_equal(e.vacant_groups(), np.nonzero(vac)[0])
    assert_canonical(e, rng.choice(np.nonzero(vac)[0], 5000, replace=False), "1M")
    e.open_groups(range(G // 4, G // 2), 700)
    e.open_groups(hosted, 800)
    assert e.count_groups() == 0
    t = BatchedRaft(G, R, seed=3)  # the twin: the same slots re-created at the same times
    t.submit_columns(kind=np.full(G // 4, capi.CMD_RECREATE, np.uint8), group=np.arange(G // 4, G // 2, dtype=np.uint32))
    t.step(700)
    t.submit_columns(kind=np.full(hosted.size, capi.CMD_RECREATE, np.uint8), group=hosted.astype(np.uint32))
    t.step(800)
    drain_all(e, t)
    compare_snapshots(e, t, "1M reopened")


@pytest.mark.parametrize("D", [pytest.param(2, id="small-2-shards"), pytest.param(3, id="small-3-shards")])
def test_shards(D):
    G, R = 1000, 3
    rng = np.random.default_rng(D)
    s = BatchedRaft(G, R, seed=4, device_ids=[0] * D)
    one = BatchedRaft(G, R, seed=4)
    gs = np.sort(rng.choice(G, 400, replace=False))
    own = rng.integers(0, R, gs.size).astype(np.uint8)
    for e in (s, one):
        e.close_groups(gs)
    assert np.array_equal(s.vacant_groups(), one.vacant_groups())
    for g0, n, lim in ((0, G, None), (300, 500, None), (0, G, 7), (480, 60, 3)):
        assert np.array_equal(s.vacant_groups(g0, n, lim), one.vacant_groups(g0, n, lim)), (g0, n, lim)
        assert np.array_equal(s.hosted_groups(g0, n, lim), one.hosted_groups(g0, n, lim)), (g0, n, lim)
    before = s.export_groups().records.tobytes()
    # a refusal in the last shard: nothing is written in the first
    last = s.shard(s.n_shards - 1).group_lo
    bad = np.union1d(gs[gs < last][:5], [np.setdiff1d(np.arange(last, G), gs)[0]])
    with pytest.raises(EngineError):
        s.open_groups(bad, 50)
    assert s.export_groups().records.tobytes() == before
    for e in (s, one):
        e.open_groups(gs, 60, self_slots=own)
    compare_snapshots(s, one, "shards")
    assert s.export_groups().records.tobytes() == one.export_groups().records.tobytes()
    # a shard's own handle takes a device list of shard-local slots
    sh = s.shard(0)
    sh.close_groups(np.arange(0, 20, 2), device=True)
    one.close_groups(np.arange(0, 20, 2))
    assert np.array_equal(s.vacant_groups(), one.vacant_groups())
