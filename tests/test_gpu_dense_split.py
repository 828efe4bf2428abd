"""The split dense tick (launch_dense_split, jg_api_core.h): the plain ack tick cut into two launches, groups [0, cut) on the
engine's stream and [cut, G) on a second one, cut = ceil(G / 2) rounded up to a workgroup of 256.  The two streams free-run,
and every other entry point must find both halves finished (JgStream joins them when the engine's stream is asked for) and
must itself be finished before the next second half starts.  JG_DENSE_SPLIT_MIN=1 is in the environment before every engine
of this file is created, so that the split is taken at these small sizes; the reference is the CPU oracle, bit for bit,
after every step.

The `launches` counter counts kernels as the work is defined, not as it is cut: a dense ack tick is ONE launch, split or
whole, plus ONE for the general-path kernel (k_dense_slow) on every tick it is scheduled behind.  So a split engine and a
whole one show the same counter, and a tick that counts two has the slow kernel behind it - which is never split."""
import ctypes as C

import numpy as np
import pytest

from josefine_amd import BatchedRaft, Command, capi
from oracle_lib import oracle_engine
from parity import DeviceSynth, compare_drains, compare_snapshots, elect_all, synth_tick_host

pytestmark = pytest.mark.gpu

NO = capi.NO_ACK


@pytest.fixture(autouse=True)
def split_from_one_group(monkeypatch):
    monkeypatch.setenv("JG_DENSE_SPLIT_MIN", "1")


def slots_of(layout, G, R):
    return None if layout == "uniform" else (np.arange(G) % R).astype(np.uint8)


def pair(G, R, make_dev=BatchedRaft, **kw):
    dev, ora = make_dev(G, R, **kw), oracle_engine(G, R, **kw)
    for e in (dev, ora):
        elect_all(e)
    compare_snapshots(dev, ora, "election")
    compare_drains(dev, ora, "election")
    return dev, ora


class Stream:
    """the synthetic ack stream: generated on the device for `dev` (parity.DeviceSynth; device=False: handed over as a host
    block, for the CPU dry run of this file's logic) and restated on the host for the oracle"""

    def __init__(self, dev, ora, mode, device=True):
        self.dev, self.ora, self.mode, self.t = dev, ora, mode, 0
        self.synth = DeviceSynth(dev) if device else None
        self.sim = np.zeros((ora.R, ora.G), dtype=np.uint64)

    def tick(self, what, others=()):
        """one dense tick on both sides (and on `others`, from the host block); every readable column, the drained rows"""
        t = self.t
        host = synth_tick_host(self.ora, self.mode, t, self.sim)
        if self.synth:
            self.synth.fill(self.mode, t)
            self.dev._check(self.dev.api.step_dense_acks_device(self.dev._h, self.synth.acks))
        else:
            self.dev.step_dense_acks(host)
        self.ora.step_dense_acks(host)
        for e in others:
            e.step_dense_acks(host)
        compare_snapshots(self.dev, self.ora, f"{what}: dense tick {t}")
        compare_drains(self.dev, self.ora, f"{what}: dense tick {t}")
        self.t += 1

    def close(self):
        if self.synth:
            self.synth.close()


# ---- 1. parity -------------------------------------------------------------------------------------------------------------
def run_parity(R, layout, make_dev=BatchedRaft, device=True, ticks=60):
    G = 1000  # cut = 512: the last workgroup of each range is partial (the first range's is not: 512 = 2 x 256 - its END is)
    dev, ora = pair(G, R, make_dev, seed=0x73706C + R, self_slots=slots_of(layout, G, R))
    s = Stream(dev, ora, mode=1, device=device)
    c0 = dev.counters()
    for _ in range(ticks):
        s.tick(f"R={R} {layout}")
    s.close()
    c1, o1 = dev.counters(), ora.counters()
    assert c1["decisions"] == o1["decisions"] and c1["dense_group_steps"] == o1["dense_group_steps"], (c1, o1)
    assert c1["launches"] - c0["launches"] == ticks  # (one per tick: see the module docstring)
    assert int(ora.read("commit").max()) > 0


@pytest.mark.parametrize("layout", ["uniform", "mixed"])
@pytest.mark.parametrize("R", [3, 5])
def test_split_tick_parity_ragged_stream(R, layout):
    run_parity(R, layout)


# ---- 2. other entry points between split ticks ------------------------------------------------------------------------------
def run_interleaved(R, make_dev=BatchedRaft, device=True, rounds=2, ticks_between=2):
    G, cut = 1000, 512
    dev, ora = pair(G, R, make_dev, seed=0x696E74 + R)
    s = Stream(dev, ora, mode=1, device=device)
    on_device = device

    def rows(cmd, groups, now):
        for e in (dev, ora):
            for g in groups:
                e.submit(int(g), cmd)
            e.step(now)

    def poll(k):
        if on_device:
            got = dev.poll(census=True, commits=dict(peek=True))
            assert got["census"]["leaders"] == int((ora.read("role") == capi.ROLE_LEADER).sum())

    def lookup(k):
        at = np.array([cut + 3, 1, G - 1, cut - 1, cut, 0], np.uint32)
        if on_device:
            got = dev.lookup(at)
            for name in ("head", "commit", "term", "fault"):
                assert np.array_equal(got[name], ora.read(name)[at]), name

    def counters(k):
        a, b = dev.counters(), ora.counters()
        assert a["decisions"] == b["decisions"], (a, b)

    def timer(k):
        if on_device:
            ms = C.c_float(-1)
            dev._check(dev.api.timer_start(dev._h))
            s.tick(f"inside the timer, round {k}")
            dev._check(dev.api.timer_stop(dev._h, C.byref(ms)))
            assert ms.value >= 0

    def drain(k):
        a, b = dev.drain_messages(), ora.drain_messages()
        assert a.tobytes() == b.tobytes()

    # groups on both sides of the cut, fresh ones every round
    def restart(k):
        rows(Command.Restart(), (7 + k, cut + 7 + k), 1000 * (k + 1))

    def request(k):  # (the restarted groups: followers now)
        assert (ora.read("role")[[7 + k, cut + 7 + k]] != capi.ROLE_LEADER).all()
        rows(Command.ClientRequest(5), (7 + k, cut + 7 + k), 1000 * (k + 1) + 1)

    def timeout(k):
        rows(Command.Timeout(), (7 + k, cut + 7 + k, 40 + k, cut + 40 + k), 1000 * (k + 1) + 2)

    for _ in range(3):
        s.tick("before anything else")
    for k in range(rounds):
        for other in (poll, lookup, counters, timer, drain, restart, request, timeout):
            other(k)
            compare_snapshots(dev, ora, f"after {other.__name__}, round {k}")
            compare_drains(dev, ora, f"after {other.__name__}, round {k}")
            for _ in range(ticks_between):
                s.tick(f"after {other.__name__}, round {k}")
    s.close()
    assert dev.counters()["decisions"] == ora.counters()["decisions"]


@pytest.mark.parametrize("R", [3, 5])
def test_other_entry_points_between_split_ticks(R):
    run_interleaved(R)


# ---- 3. sizes around the workgroup and the cut ------------------------------------------------------------------------------
def run_degenerate(G, monkeypatch, make_dev=BatchedRaft, device=True, ticks=12):
    """G = 1, 255, 256: the second range would be empty - one launch; 257 and 513: a second range of ONE group"""
    R = 3
    kw = dict(seed=0x646567 + G, self_slots=slots_of("mixed", G, R))
    dev, ora = pair(G, R, make_dev, **kw)
    monkeypatch.setenv("JG_DENSE_SPLIT_MIN", "0")  # (read when the engine is created)
    whole = make_dev(G, R, **kw)
    monkeypatch.setenv("JG_DENSE_SPLIT_MIN", "1")
    elect_all(whole)
    whole.drain_messages(), whole.drain_applies(), whole.drain_faults()
    s = Stream(dev, ora, mode=1, device=device)
    c0, w0 = dev.counters(), whole.counters()
    for _ in range(ticks):
        s.tick(f"G={G}", others=(whole,))
        compare_snapshots(whole, dev, f"G={G} whole against split, tick {s.t - 1}")
    s.close()
    c1, w1 = dev.counters(), whole.counters()
    assert c1["launches"] - c0["launches"] == w1["launches"] - w0["launches"] == ticks
    assert c1["decisions"] == w1["decisions"] == ora.counters()["decisions"]


@pytest.mark.parametrize("G", [1, 255, 256, 257, 513])
def test_sizes_around_the_workgroup_and_the_cut(G, monkeypatch):
    run_degenerate(G, monkeypatch)


# ---- 4. the general path on both sides of the cut ---------------------------------------------------------------------------
def run_faults(make_dev=BatchedRaft):
    """R = 5: lag fields of 10 bits (escape above 1021 blocks), a quorum of three.  Per range one group whose acks come to lie
    above the head - the third forged ack moves the quorum there: chain.commit panics (chain.rs:197-202) - and one whose
    silent follower falls 1200 blocks behind: its lag field escapes to the wide column.  Neither is served in lag space: the
    kernel takes them through its in-kernel general path and says so (cold_seen); the next synchronising call - here the
    reads of the comparison - schedules k_dense_slow behind every later tick, and such a tick is not split: 2 launches."""
    G, R, cut = 1000, 5, 512
    dev, ora = pair(G, R, make_dev, seed=0x666C74)
    forged, silent = (5, cut + 5), (9, G - 1)
    launches = []

    def tick(t, what):
        head = ora.read("head").astype(np.uint64)
        acks = np.full((R, G), NO, dtype=np.uint64)
        acks[0] = 1
        acks[1:] = head  # everybody acknowledges everything so far
        acks[0, list(silent)] = 600
        acks[4, list(silent)] = NO
        for k in (1, 2, 3):
            if t >= k:
                acks[k, list(forged)] = 10**6
        c0 = dev.counters()["launches"]
        dev.step_dense_acks(acks)
        ora.step_dense_acks(acks)
        launches.append(dev.counters()["launches"] - c0)
        compare_snapshots(dev, ora, f"{what} (tick {t})")
        compare_drains(dev, ora, f"{what} (tick {t})")  # the fault rows: (step, group) order

    tick(0, "all in lag space")
    assert launches == [1] and not ora.read("fault").any()
    tick(1, "the first forged ack: above the head, no quorum; the silent follower is 1200 behind: escaped")
    assert launches[1] == 1  # (the kernel that met the general path was still a plain one ...)
    tick(2, "the second forged ack")
    assert launches[2] == 2  # (... and the one after the synchronisation has the slow kernel behind it)
    tick(3, "the third forged ack: the quorum is above the head")
    tick(4, "the dead groups ignore everything")
    assert launches[3:] == [2, 2]
    fault = ora.read("fault")
    assert (fault[list(forged)] == capi.FAULT_COMMIT_MISSING_BLOCK).all() and np.count_nonzero(fault) == 2


def test_general_path_on_both_sides_of_the_cut():
    run_faults()
