"""Wide terms and clocks: the bases, the set-up helpers and the drivers of tests/test_wide_values*.py.

Every other test starts its clock at 0 and its terms at 0; a caller passes wall-clock milliseconds (above 2^40) and the
terms of a long-lived cluster.  The drivers here put an engine and its reference into the SAME wide state through ordinary
rows - a Recreate at the clock base, then a Heartbeat (or a candidate's VoteRequest) at the term base - and go on from
there with the suite's own comparisons (parity.compare_snapshots / compare_drains).  A driver takes the factory of the
engine under test, so the device, the emulated device and the host-compiled device source (tests/host_compiled.py) run
the same cases.

What a Heartbeat cannot do: it leaves the follower with a vote (follower.rs:187), and a follower that has voted never
campaigns (follower.rs:249).  Where a case needs followers that can time out, or leaders, at a wide term,
the groups get there as the reference allows: Timeout (candidate), then a VoteRequest at the wide term from a peer
(candidate.rs:71-88: Raft::term, follower again, no vote) - `unvoted_at` - and, for leaders, `elect_wide` on top of it."""
import numpy as np

from josefine_amd import Command, capi
from parity import compare_drains, compare_snapshots

M64 = (1 << 64) - 1
BOUND = 1 << 32

C32 = 2**32 - 450          # with dt = 100 ms the clock crosses 2^32 in the fifth round
CEPOCH = 1_760_000_000_000  # wall-clock milliseconds
C63 = 2**63 - 450
CWRAP = 2**64 - 450        # a translation check only: the device at now + CWRAP, the reference at now

T32 = 2**32 - 3
THI = (7 << 32) + 5
T63 = 2**63 - 3

PAIRS = [(C32, T32), (CEPOCH, THI), (C63, T63)]
PAIR_IDS = ["c32-t32", "cepoch-thi", "c63-t63"]
TIMERS = ("election_time", "heartbeat_time")
NO = capi.NO_ACK


def drain(e):
    return e.drain_messages(), e.drain_applies(), e.drain_faults()


def _groups(e, groups):
    return np.arange(e.G, dtype=np.uint32) if groups is None else np.ascontiguousarray(groups, dtype=np.uint32)


def _peer(e, g, k=1):
    """the id of the member k slots after the own one, per listed group"""
    ids = np.array(e.node_ids, dtype=np.uint32)
    return ids[(e.read("self_slot")[g].astype(np.int64) + k) % e.R]


def raise_clock(engines, base):
    """Recreate on every group at `base`: every timer sits at `base` (Raft::new on an empty store)"""
    for e in engines:
        e.apply_all(Command.Recreate(), int(base) & M64)


def raise_term(engines, term, leader=None, now=0, groups=None):
    """one Heartbeat(term, 0, leader) row to every (listed) group, stepped at `now`: the followers adopt the term
    (follower.rs:178-217) and the leader.  term: one value or one per listed group; leader: a member id (default: the
    member after the own slot)"""
    for e in engines:
        g = _groups(e, groups)
        n = len(g)
        frm = _peer(e, g) if leader is None else np.full(n, leader, np.uint32)
        e.submit_columns(np.full(n, capi.CMD_HEARTBEAT, np.uint8), g, from_=frm, term=np.broadcast_to(np.asarray(term, dtype=np.uint64), (n,)),
                         id=np.zeros(n, np.uint64))
        e.step(int(now) & M64)


def unvoted_at(engines, term, now=0, groups=None):
    """followers at `term` that have NOT voted: Timeout (a fresh follower campaigns), then a peer's VoteRequest at `term`
    (> the candidate's: Raft::term, follower again, nothing granted - candidate.rs:71-88)"""
    for e in engines:
        g = _groups(e, groups)
        n = len(g)
        e.submit_columns(np.full(n, capi.CMD_TIMEOUT, np.uint8), g)
        e.step(int(now) & M64)
        t = np.broadcast_to(np.asarray(term, dtype=np.uint64), (n,))
        e.submit_columns(np.full(n, capi.CMD_VOTE_REQUEST, np.uint8), g, from_=_peer(e, g), term=t, id=np.zeros(n, np.uint64), aux=t)
        e.step(int(now) & M64)


def elect_wide(engines, term, now=0, groups=None):
    """leaders AT `term`: unvoted followers at term - 1, Timeout (the campaign raises the term), granted VoteResponses from
    the next R / 2 members (traces.elect_all, for a subset and at a clock)"""
    for e in engines:
        g = _groups(e, groups)
        n = len(g)
        unvoted_at([e], np.asarray(term, dtype=np.uint64) - np.uint64(1), now, g)
        e.submit_columns(np.full(n, capi.CMD_TIMEOUT, np.uint8), g)
        e.step(int(now) & M64)
        for k in range(1, e.R // 2 + 1):
            e.submit_columns(np.full(n, capi.CMD_VOTE_RESPONSE, np.uint8), g, from_=_peer(e, g, k), term=np.ones(n, np.uint64), flag=np.ones(n, np.uint8))
            e.step(int(now) & M64)


def compare_shifted(dev, ora, shift, what):
    """every column equal, the two timers equal after taking `shift` off the device's (mod 2^64)"""
    if not shift:
        return compare_snapshots(dev, ora, what)
    compare_snapshots(dev, ora, what, fields=[f for f in capi.FIELD_NAMES if f not in TIMERS])
    for name in TIMERS:
        a, b = dev.read(name), ora.read(name)
        live = np.ones(len(a), bool) if name == "election_time" else (ora.read("role") == capi.ROLE_LEADER)  # (heartbeat_time: Leader's own field)
        with np.errstate(over="ignore"):
            back = a - np.uint64(shift)
        bad = np.nonzero((back != b) & live)[0]
        assert not len(bad), f"{what}: {name} - shift differs at groups {bad[:8]}: hip={a[bad[:8]]} oracle={b[bad[:8]]}"


def cmp_cols(a, b, what):
    for k in a:
        if not np.array_equal(a[k], b[k]):
            bad = np.argwhere(a[k] != b[k])[:6]
            raise AssertionError(f"{what}: outbox column {k} differs at {bad.tolist()}: hip={[a[k][tuple(i)] for i in bad]} oracle={[b[k][tuple(i)] for i in bad]}")


def own_slots(G, R, layout):
    return {"slot0": None, "last": np.full(G, R - 1, np.uint8), "mixed": (np.arange(G) % R).astype(np.uint8)}[layout]


def sides(values):
    """which sides of 2^32 a column of values lies on"""
    v = np.asarray(values, dtype=np.uint64)
    return bool((v < np.uint64(BOUND)).any()), bool((v >= np.uint64(BOUND)).any())


# ---- item 2: the dense halves ------------------------------------------------------------------------------------------
# the leader half's schedule, in ms after the base (heartbeat timeout 100).  Three classes of groups are elected at base,
# base + 200 and base + 201; with now - heartbeat_time > 100 a leader beats and its heartbeat_time becomes now:
#   tick at  300 301 401 402 | 500 501 502 702 | 801 802 803 1103
#   class 0  300*  1 101*  1 |  99 100 101* 200*|  99 100 101* 300*     (* = a beat)
#   class 1  100 101* 100 101*|  98  99 100 300*|  as class 0
#   class 2   99 100 200*  1 |  as class 0
# For C32 (2^32 = base + 450) every one of hb - 1, hb, hb + 1 and 3 hb occurs with both times below 2^32, with the
# heartbeat_time below and now at or above it (the subtraction borrows across the halves), and with both above.
LEADER_ELECTIONS = (0, 200, 201)
LEADER_TICKS = (300, 301, 401, 402, 500, 501, 502, 702, 801, 802, 803, 1103)
HB = 100


def leader_half_case(make, make_ref, R, base, term, layout, G=192, ref_base=None):
    """item 2, the leader half; ref_base: the reference's clock base where it differs (the wrap: item 5)"""
    from dense_node import random_leader_inbox
    ref_base = base if ref_base is None else ref_base
    shift = (base - ref_base) & M64
    slots = own_slots(G, R, layout)
    kw = dict(seed=21, flags=capi.CFG_SEPARATE_COMMIT_KEY, self_slots=slots, heartbeat_timeout_ms=HB)
    dev, ora = make(G, R, **kw), make_ref(G, R, **kw)
    sides_ = [(dev, base), (ora, ref_base)]
    cls = np.arange(G) % 3
    for e, b in sides_:
        raise_clock([e], b)
        for c, off in enumerate(LEADER_ELECTIONS):
            elect_wide([e], term, b + off, np.nonzero(cls == c)[0])
    compare_shifted(dev, ora, shift, "elected")
    compare_drains(dev, ora, "elected")
    assert (ora.read("role") == capi.ROLE_LEADER).all() and (ora.read("term") == np.uint64(term)).all()
    rng = np.random.default_rng(R)
    sl = ora.read("self_slot")
    seen = set()
    for t, off in enumerate(LEADER_TICKS):
        now = ref_base + off
        led = (ora.read("role") == capi.ROLE_LEADER) & (ora.read("fault") == 0)
        hbt, nw = ora.read("heartbeat_time")[led], np.uint64(now & M64)
        side = np.where(nw < np.uint64(BOUND), "below", np.where(hbt < np.uint64(BOUND), "across", "above"))
        seen |= set(zip((nw - hbt).tolist(), side.tolist()))
        acks, hbr_has, hbr_commit = random_leader_inbox(rng, G, R, sl, ora.read("head"))
        oa = dev.step_dense_leader((base + off) & M64, acks, hbr_has, hbr_commit, tick=True)
        ob = ora.step_dense_leader(now & M64, acks, hbr_has, hbr_commit, tick=True)
        cmp_cols(oa, ob, f"R={R} leader tick {t}")
        compare_shifted(dev, ora, shift, f"R={R} leader tick {t}")
        compare_drains(dev, ora, f"R={R} leader tick {t}")
    # a leader whose heartbeat_time is stale by MORE than 2^32 ms: the low halves alone say 50 ms (not due); it beats
    now = ref_base + LEADER_TICKS[-1] + BOUND + 50
    led = (ora.read("role") == capi.ROLE_LEADER) & (ora.read("fault") == 0)
    assert led.sum() > G // 2 and (np.uint64(now & M64) - ora.read("heartbeat_time")[led] == np.uint64(BOUND + 50)).all()
    acks = np.full((R, G), NO, np.uint64)
    acks[sl, np.arange(G)] = 0
    oa = dev.step_dense_leader((now + shift) & M64, acks, tick=True)
    ob = ora.step_dense_leader(now & M64, acks, tick=True)
    cmp_cols(oa, ob, f"R={R} stale leaders' tick")
    compare_shifted(dev, ora, shift, f"R={R} stale leaders' tick")
    compare_drains(dev, ora, f"R={R} stale leaders' tick")
    assert (ob["hb_commit"][led] != np.uint64(NO)).all() and (ora.read("heartbeat_time")[led] == np.uint64(now & M64)).all()
    want = (HB - 1, HB, HB + 1, 3 * HB)
    assert {d for d, _ in seen} >= set(want), seen
    if ref_base < BOUND <= ref_base + LEADER_TICKS[-1]:
        missing = [(d, s) for d in want for s in ("below", "across", "above") if (d, s) not in seen]
        assert not missing, missing
    assert int(ora.read("commit").max()) > 0 and (ora.read("term")[ora.read("fault") == 0] == np.uint64(term)).all()
    return dev, ora


BEAT_CLASSES = ("F-1", "F", "F+1", "F^2^32", "F&0xffffffff")


def beat_terms(F, k):
    """the beat term of class k (an index into BEAT_CLASSES, per group) for followers at term F"""
    F = np.asarray(F, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return np.choose(k, [F - np.uint64(1), F, F + np.uint64(1), F ^ np.uint64(BOUND), F & np.uint64(0xFFFFFFFF)]).astype(np.uint64)


def follower_half_case(make, make_ref, R, base, term, layout, G=192, ref_base=None):
    """item 2, the follower half.  Groups 0 mod 2 follow (a Heartbeat: they have voted), groups 1 mod 2 have not voted; of
    those, groups 1 mod 4 never get mail - their election timers run out.  Followers start at `term` or `term` + 2^32, so
    that the class F ^ 2^32 changes the high half in both directions."""
    ref_base = base if ref_base is None else ref_base
    shift = (base - ref_base) & M64
    slots = own_slots(G, R, layout)
    kw = dict(seed=31, flags=capi.CFG_SEPARATE_COMMIT_KEY, self_slots=slots, election_timeout_ms=(500, 1000))
    dev, ora = make(G, R, **kw), make_ref(G, R, **kw)
    g = np.arange(G)
    with np.errstate(over="ignore"):
        F0 = np.uint64(term) + np.where((g // 2) % 2 == 1, np.uint64(BOUND), np.uint64(0)).astype(np.uint64)
    voted, timer_only = g % 2 == 0, g % 4 == 1
    for e, b in ((dev, base), (ora, ref_base)):
        raise_clock([e], b)
        unvoted_at([e], F0[~voted], b, g[~voted])
        raise_term([e], F0[voted], None, b, g[voted])
    compare_shifted(dev, ora, shift, "followers")
    compare_drains(dev, ora, "followers")
    assert (ora.read("role") == capi.ROLE_FOLLOWER).all() and np.array_equal(ora.read("term"), F0) and np.array_equal(ora.read("has_voted") != 0, voted)
    rng = np.random.default_rng(100 + R)
    accepted, refused = np.zeros(5, np.int64), np.zeros(5, np.int64)
    kinds_seen, timer_at = set(), set()
    campaigned = np.zeros(G, bool)
    now = ref_base
    step = 0
    for stage in range(4):
        # the group whose timer this stage walks across: the first, the middle, the last of those still to fire, the first again
        role, fault, voted_now = ora.read("role"), ora.read("fault"), ora.read("has_voted") != 0
        et, to = ora.read("election_time"), ora.read("election_timeout").astype(np.uint64)
        can = timer_only & (fault == 0) & (role != capi.ROLE_LEADER) & ((role == capi.ROLE_CANDIDATE) | ~voted_now)
        due = np.where(can, (et + to).astype(np.uint64), np.uint64(M64))
        due = np.where(due > np.uint64(now + 1), due, np.uint64(M64))
        order = np.argsort(due, kind="stable")
        n_can = int((due != np.uint64(M64)).sum())
        assert n_can > 0, stage
        target = order[{0: 0, 1: n_can // 2, 2: n_can - 1, 3: 0}[stage]]
        for d in (-1, 0, 1):
            now = int(due[target]) + d
            term_now, head, commit = ora.read("term"), ora.read("head"), ora.read("commit")
            k = ((g // 4 + step) % 5).astype(np.int64)
            beat = beat_terms(term_now, k)
            m = (g // 4 + g % 4 + 2 * step) % 4  # 0: a Heartbeat only, 1: an AppendEntries only, 2: both, 3: nothing
            m = np.where(timer_only, 3, m)
            has_hb, has_ae = (m == 0) | (m == 2), (m == 1) | (m == 2)
            hbc = np.where(has_hb, np.minimum(head, commit + rng.integers(0, 3, G).astype(np.uint64)), np.uint64(NO)).astype(np.uint64)
            ae_n = np.where(has_ae, rng.integers(0, 4, G), capi.AE_NONE).astype(np.uint8)
            other = rng.random(G) < 0.2  # a second sender: what a follower that voted for the first one refuses
            sender = np.where(other, _peer(ora, g, 2), _peer(ora, g, 1)).astype(np.uint32)
            inbox = dict(leader=sender, term=beat, hb_commit=hbc, ae_from=head.astype(np.uint64), ae_n=ae_n)
            pre = dict(role=ora.read("role"), fault=ora.read("fault"), et=ora.read("election_time"), to=ora.read("election_timeout").astype(np.uint64),
                       voted=ora.read("has_voted") != 0)
            oa = dev.step_dense_follower((now + shift) & M64, **inbox, tick=True)
            ob = ora.step_dense_follower(now & M64, **inbox, tick=True)
            cmp_cols(oa, ob, f"R={R} follower step {step}")
            compare_shifted(dev, ora, shift, f"R={R} follower step {step}")
            compare_drains(dev, ora, f"R={R} follower step {step}")
            # what the reference made of it
            mail = (has_hb | has_ae) & (pre["fault"] == 0) & (pre["role"] == capi.ROLE_FOLLOWER)
            took = mail & (ora.read("fault") == 0) & (ora.read("has_voted") != 0) & (ora.read("voted_for") == sender) & (ora.read("term") == beat)
            for c in range(5):
                accepted[c] += int((took & (k == c)).sum())
                refused[c] += int((mail & ~took & (k == c)).sum())
            kinds_seen |= set(np.unique(m[mail]).tolist())
            quiet = (m == 3) & (pre["fault"] == 0) & (pre["role"] != capi.ROLE_LEADER)
            with np.errstate(over="ignore"):
                over = (np.uint64(now & M64) - pre["et"] - pre["to"]).astype(np.int64)
            timer_at |= set(int(x) for x in over[quiet] if -1 <= x <= 1)
            fired = quiet & (over > 0) & ((pre["role"] == capi.ROLE_CANDIDATE) | ~pre["voted"])
            assert (ora.read("election_time")[fired] == np.uint64(now & M64)).all() and (ora.read("role")[fired] == capi.ROLE_CANDIDATE).all()
            assert (ora.read("election_time")[quiet & (over <= 0)] == pre["et"][quiet & (over <= 0)]).all()
            campaigned |= fired
            step += 1
    assert (accepted > 0).all() and (refused > 0).all(), (BEAT_CLASSES, accepted, refused)
    assert kinds_seen >= {0, 1, 2}, kinds_seen
    assert timer_at == {-1, 0, 1}, timer_at
    assert campaigned.sum() * 5 >= G, int(campaigned.sum())
    if term < BOUND:
        assert sides(ora.read("term")) == (True, True)
    if ref_base < BOUND <= now:
        assert sides(ora.read("election_time")) == (True, True)
    return dev, ora


# ---- item 3: the node step ---------------------------------------------------------------------------------------------
def node_pair(make, make_ref, G, R, base, term, seed, **kw):
    """tests/test_node_step.py's mixed population at a wide clock and term: 60 % of the groups led (at `term`), of the others
    half follow at `term` with a vote, half without"""
    dev, ora = make(G, R, seed=seed, **kw), make_ref(G, R, seed=seed, **kw)
    rng = np.random.default_rng(seed)
    led = rng.random(G) < 0.6
    g = np.arange(G)
    for e in (dev, ora):
        raise_clock([e], base)
        elect_wide([e], term, base, g[led])
        unvoted_at([e], term, base, g[~led & (g % 2 == 1)])
        raise_term([e], term, None, base, g[~led & (g % 2 == 0)])
    compare_snapshots(dev, ora, "node set-up")
    compare_drains(dev, ora, "node set-up")
    assert (ora.read("term") == np.uint64(term)).all() and np.array_equal(ora.read("role") == capi.ROLE_LEADER, led)
    return dev, ora, rng


def commit_compact(dev, cols, packed, id32=True):
    """a batch through the compact bus formats: JG_COL_PACKED_KIND | JG_COL_ID32 | JG_COL_UNCHECKED (tests/test_node_step.py)"""
    import ctypes as C
    n, nb = len(cols["kind"]), len(cols["blk_id"])
    c = capi.CmdCols()
    dev._check(dev.api.submit_reserve(dev._h, n, nb, C.byref(c)))

    def view(ptr, dt, m):
        return np.frombuffer((C.c_char * (max(m, 1) * np.dtype(dt).itemsize)).from_address(ptr), dtype=dt)[:m]
    view(c.kind, np.uint8, n)[:] = packed
    view(c.group, np.uint32, n)[:] = cols["group"]
    view(c.term, np.uint64, n)[:] = cols["term"]
    view(c.id, np.uint32 if id32 else np.uint64, n)[:] = cols["id"].astype(np.uint32 if id32 else np.uint64)
    view(c.aux, np.uint64, n)[:] = cols["aux"]
    if nb:
        view(c.blk_id, np.uint64, nb)[:] = cols["blk_id"]
        view(c.blk_next, np.uint64, nb)[:] = cols["blk_next"]
    dev._check(dev.api.submit_commit(dev._h, n, nb, capi.COL_TERM | capi.COL_AUX | capi.COL_UNCHECKED | capi.COL_PACKED_KIND | (capi.COL_ID32 if id32 else 0)))


def fsm_in_partition_order(rows):
    """fsm rows per partition in emission order (the order between partitions is the step's representation)"""
    return rows[np.argsort(rows["group"], kind="stable")]


def node_step_case(make, make_ref, R, base, term, compact=False, keep=False, G=300, T=10):
    """item 3: the adversarial row traffic of tests/node_step.py through jg_step_node at a wide clock and term - plain rows
    or the compact bus formats (ids 32-bit on the bus, terms wide), one step or two in flight - against the reference's
    arrival-order step: outbox, fsm rows, state, drains"""
    from node_step import compare_outboxes, node_traffic, pack_kind
    dev, ora, rng = node_pair(make, make_ref, G, R, base, term, seed=40 + R, flags=capi.CFG_SEPARATE_COMMIT_KEY, election_timeout_ms=(700, 1500))
    ids = list(ora.node_ids)
    want = []
    general = wide_rows = 0

    def check(t, a):
        b, rows = want[t]
        compare_outboxes(a, b, f"node step {t}")
        for fn in ("drain_messages", "drain_applies", "drain_faults"):
            got = getattr(dev, fn)()
            if fn == "drain_applies":
                got, exp = fsm_in_partition_order(got), fsm_in_partition_order(rows[fn])
            else:
                exp = rows[fn]
            assert got.shape == exp.shape and got.tobytes() == exp.tobytes(), f"node step {t}: {fn}: {len(got)} rows against {len(exp)}"

    for t in range(T):
        now = base + 100 * (t + 1)
        cols = node_traffic(rng, ora, token0=1000 * t, p_noise=0.03 if t % 3 else 0.0, p_reorder=0.08 if t % 3 else 0.0)
        if compact:
            packed, said = pack_kind(cols, ids, R)
            cols = dict(cols, from_=said, flag=(cols["flag"] != 0).astype(np.uint8), id=cols["id"] & np.uint64(0xFFFFFFFF))
            commit_compact(dev, cols, packed)
        else:
            dev.submit_columns(**cols)
        wide_rows += int((cols["term"] >= np.uint64(BOUND - 8)).sum())
        ora.submit_columns(**cols)
        b = ora.step_node(now)
        want.append((b, {fn: getattr(ora, fn)() for fn in ("drain_messages", "drain_applies", "drain_faults")}))
        general += b["rows_general"] > 0
        if keep:
            dev.step_node_begin(now, async_=True, keep=True)
            if t:
                check(t - 1, dev.node_outbox())
        else:
            check(t, dev.step_node(now))
            compare_snapshots(dev, ora, f"node step {t}")
    if keep:
        check(T - 1, dev.node_outbox())
    compare_snapshots(dev, ora, "after the last node step")
    assert general > 2 and wide_rows > G
    assert (ora.read("term")[ora.read("fault") == 0] >= np.uint64(term)).sum() > G // 2
    return dev, ora


# ---- item 4: clusters --------------------------------------------------------------------------------------------------
def wide_cluster_nodes(make, G, R, base, term, lead=0, seed=5):
    """the R engines of dense_node.DenseCluster (engine r hosts replica slot r) at `base`, node `lead` leading every group at
    `term`; the others have not heard of it yet (their first Heartbeat carries the term)"""
    from josefine_amd.traces import elect_all
    nodes = [make(G, R, seed=seed + r, self_slots=np.full(G, r, np.uint8), flags=capi.CFG_SEPARATE_COMMIT_KEY) for r in range(R)]
    elect_all(nodes[lead])  # (as DenseCluster's constructor: the timeout draws of the two sides stay in step)
    raise_clock(nodes, base)
    elect_wide([nodes[lead]], term, base)
    for n in nodes:
        drain(n)
    return nodes


def wide_cluster(cls, make, G, R, base, term, lead=0, seed=5):
    """a tests/dense_node.py cluster (DenseCluster / RoutedCluster) whose nodes start as wide_cluster_nodes'"""
    cl = cls(make, G, R, seed=seed, lead=lead)
    raise_clock(cl.nodes, base)
    elect_wide([cl.nodes[lead]], term, base)
    for n in cl.nodes:
        drain(n)
    cl.now = base
    return cl


def boundary(term):
    """the boundary a term base sits just below: 2^32 for 2^32 - 3, 2^63 for 2^63 - 3"""
    return BOUND if term < BOUND else 1 << 63


def _merge_rows(a, b):
    """two per-node row sets for one round as one, group-sorted (a's rows of a group before b's)"""
    if a is None or b is None:
        return b if a is None else a
    keys = set(a) | set(b)
    na, nb = len(a["kind"]), len(b["kind"])
    dt = dict(kind=np.uint8, group=np.uint32, from_=np.uint32, term=np.uint64, id=np.uint64, aux=np.uint64, flag=np.uint8)
    cat = {k: np.concatenate([a.get(k, np.zeros(na, dt[k])), b.get(k, np.zeros(nb, dt[k]))]).astype(dt[k]) for k in keys}
    order = np.argsort(cat["group"], kind="stable")
    return {k: v[order] for k, v in cat.items()}


def routed_cluster_case(R, G, base, term, words=False, any_leader=False, T=40, percent=25, repair_after=3):
    """item 4, the routed cluster: jg_dense_cluster_round_routed (rows, or the election's traffic as mailbox words) against
    the Python-routed cluster over oracle engines (dense_node.RoutedCluster; any_leader - jg_dense_cluster_create with
    lead=None - dense_node.AnyLeaderCluster), every column of every node after every round, from a wide clock, every
    leader seated at `term`, under failures at `percent` % per round: the failure and repair schedule of
    josefine_amd.traces.FailureRepairTrace, or for per-partition leadership its counterpart any_failure_rows with
    re-created groups (that schedule names one lead node).
    A restart puts a replica's term back to 0 (State::default()), so the elections of those schedules run at small terms,
    while the voters that were not restarted answer at wide ones.  The elections that CROSS the boundary are campaigns of
    their own: one group in eight starts without a leader, every replica without a vote at boundary - 1 (groups 3 mod 8) or
    boundary - 2 (groups 7 mod 8); node 1's Timeout in round 0 raises the term to the boundary resp. to just below it, its
    VoteRequests (granted only if last_term arrives whole: follower.rs:97-101), the grants and the winner's Heartbeat all
    travel through the transport.  Asserted on the oracle: leaders elected DURING the run on both sides of the boundary,
    and at least G / 4 elections won through the transport.  (The campaigns are counted in round 3; a failure that hits such
    a group before that takes it out of the count, not out of the comparison.)
    Returns (device nodes, oracle cluster, library cluster, appends of the last round, now)."""
    from josefine_amd import BatchedRaft, DenseCluster as LibCluster
    from josefine_amd.traces import FailureRepairTrace, any_failure_rows, elect_all
    from dense_node import AnyLeaderCluster, RoutedCluster
    from oracle_lib import oracle_engine
    g = np.arange(G)
    bound = boundary(term)
    at, under = g % 8 == 3, g % 8 == 7
    camp = at | under
    leader_of = np.where(camp, 1, g % R if any_leader else 0)

    def start(nodes):
        raise_clock(nodes, base)
        for n in range(R):
            mine = ~camp & (leader_of == n)
            if mine.any():
                elect_wide([nodes[n]], term, base, g[mine])
        unvoted_at(nodes, bound - 1, base, g[at])
        unvoted_at(nodes, bound - 2, base, g[under])
        for n in nodes:
            drain(n)

    ora = AnyLeaderCluster(oracle_engine, G, R, seed=5) if any_leader else RoutedCluster(oracle_engine, G, R, seed=5)
    nodes = [BatchedRaft(G, R, seed=5 + r, self_slots=np.full(G, r, np.uint8), flags=capi.CFG_SEPARATE_COMMIT_KEY) for r in range(R)]
    if not any_leader:
        elect_all(nodes[0])  # (as RoutedCluster's constructor: the timeout draws of the two sides stay in step)
    start(ora.nodes)
    start(nodes)
    ora.now = base
    for n in range(R):
        compare_snapshots(nodes[n], ora.nodes[n], f"cluster set-up node {n}")
    lib = LibCluster(nodes, lead=None if any_leader else 0, vote_words=words)
    lib.set_appends(1)
    tr = None if any_leader else FailureRepairTrace(99, G, R, percent, repair_after, node_ids=ora.member_ids)
    appends = np.ones(G, np.uint64)
    won = won_at = won_under = 0
    failed_at = np.full(G, -1)
    for t in range(T):
        lists = []
        if any_leader:
            inj, failing = any_failure_rows(99, t, G, R, percent, leader_of, whole_group=True, recreate=True, skip=camp if t <= 3 else None) if t >= 3 else ([None] * R, [])
            # an election after a failure takes three rounds: the next replica leads then, at term 1
            done = np.nonzero(failed_at == t - 3)[0]
            lead_now = (leader_of[done] + 1) % R
            roles = np.stack([n.read("role") for n in ora.nodes])
            won += int((roles[lead_now, done] == capi.ROLE_LEADER).sum())
            leader_of[done] = lead_now
            failing = failing[failed_at[failing] < 0] if len(failing) else failing
            failed_at[done] = -1
        else:
            inj, failing, repaired = tr.rows(t)
            appends = tr.appends()
            lists = [nodes[0].upload_u32(x) if len(x) else None for x in (failing, repaired)]
            if lists[0] is not None:
                lib.withdraw_appends(lists[0].ptr, len(failing))
            if lists[1] is not None:
                lib.offer_appends(lists[1].ptr, len(repaired), 1)
        inj = list(inj)
        if any_leader and len(failing):
            failed_at[failing] = t
        if t == 0:  # the campaigns at the boundary: node 1's Timeout
            inj[1] = _merge_rows(inj[1], dict(kind=np.full(int(camp.sum()), capi.CMD_TIMEOUT, np.uint8), group=g[camp].astype(np.uint32)))
        up = [None if c is None else nodes[n].upload_rows(**c) for n, c in enumerate(inj)]
        st = lib.round_routed((base + (t + 1) * 100) & M64, up)
        ora.round(appends, inject=inj)
        for n in range(R):
            compare_snapshots(nodes[n], ora.nodes[n], f"routed round {t} node {n}")
        pending = [ora.pending(n) for n in range(R)]
        assert (st["delivered"] == pending) if not words else all(a <= b for a, b in zip(st["delivered"], pending)), (t, st["delivered"], pending)
        if not any_leader:
            won += int((ora.nodes[0].read("role")[repaired] == capi.ROLE_LEADER).sum())
        if t == 3:  # (Timeout in round 0, the VoteRequests delivered in round 1, the grants in round 2: elected)
            role1, term1 = ora.nodes[1].read("role"), ora.nodes[1].read("term")
            won_at = int(((role1 == capi.ROLE_LEADER) & (term1 == np.uint64(bound)) & at).sum())
            won_under = int(((role1 == capi.ROLE_LEADER) & (term1 == np.uint64(bound - 1)) & under).sum())
        for rows in up + lists:
            if rows is not None:
                rows.free()
    # leaders elected during the run through the transport: at the boundary (the campaign's term + 1 crossed it), just below
    # it, and - the schedule's - at small terms
    assert won_at > 0 and won_under > 0 and won > 0, (won_at, won_under, won)
    assert won + won_at + won_under >= G // 4, (won, won_at, won_under)
    return nodes, ora, lib, appends, base + T * 100


def check_cluster_drains(nodes, ora):
    for n in range(len(nodes)):
        got, want = nodes[n].drain_messages(), ora.kept[n]
        assert got.tobytes() == want.tobytes(), (n, len(got), len(want))
        assert nodes[n].drain_faults().tobytes() == ora.nodes[n].drain_faults().tobytes()
        assert nodes[n].drain_applies().tobytes() == ora.nodes[n].drain_applies().tobytes()
