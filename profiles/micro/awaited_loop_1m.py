"""A loop of kept node steps at 1 M slots, R = 5, every slot a leader, compact bus (JG_NODE_COMMON_AE | JG_NODE_FSM_FUSED), two
ticks in flight, with the completion feed at 1 M waiters of which 1 % are done per tick (10 486 fresh waiters a tick whose
block is committed already; the table stays at 1 M, the others wait).  One mode per process:

  plain    no attachment: jg_step_node, the older step's outbox viewed, its rows drained by view
  awaited  jg_step_node_awaited on every step: the tick's waiters registered and the watch made behind the step
  cancelled  awaited, and a cancel of 16 exact tokens travels with every step (ABI v24): 16 of the waiters that wait are
           withdrawn and leave with the tick's watch, beside the 1 %
  sync     what a loop could do before ABI v23: the outstanding step viewed first (the three calls are refused while a
           kept step is outstanding), then jg_engine_await_blocks + jg_engine_watch_completions - one tick in flight

The steps carry no inbound rows (the tick's kernels, its outbox columns and fsm rows on their way home are what is
timed; the row passes are not).  Every call goes through ctypes without a host copy of the columns.  Prints one JSON line:
the median and the quartiles of the wall time per tick.  Run by profiles/micro/awaited_loop_1m.sh."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(mode, slots=1 << 20, ticks=80, warmup=16):
    import numpy as np
    from josefine_amd import BatchedRaft, capi
    from josefine_amd.traces import elect_all
    G, R, W = slots, 5, slots  # (a smaller size as the second argument: a dry run)
    per_tick = W // 100
    e = BatchedRaft(G, R, seed=1, flags=capi.CFG_SEPARATE_COMMIT_KEY)  # (a leader's Tick then scans no commit key: no Q9 fault)
    elect_all(e, 10)
    e.drain_messages(), e.drain_applies(), e.drain_faults()
    acks = np.full((R, G), capi.NO_ACK, np.uint64)
    for appends in (2, 0):  # two blocks everywhere, acknowledged by everybody a tick later: commit = head = 2
        acks[:] = capi.NO_ACK
        acks[0, :] = appends
        acks[1:, :] = e.read("head")
        e.step_dense_acks(acks)
        e.drain_messages(), e.drain_applies(), e.drain_faults()
    assert (e.read("commit") == 2).all()
    rng = np.random.default_rng(2)
    e.open_waiters(W + 4 * per_tick)
    e.await_blocks(rng.integers(0, G, W - per_tick), 1 << 40, np.arange(W - per_tick))  # they wait
    api, h = e.api, e._h
    flags = capi.NODE_LEADER_HALF | capi.NODE_TICK | capi.NODE_ASYNC | capi.NODE_KEEP | capi.NODE_COMMON_AE | capi.NODE_FSM_FUSED
    fresh = np.zeros(per_tick, capi.AWAIT_ROW_DTYPE)
    out = np.zeros(2 * per_tick, capi.DONE_ROW_DTYPE)
    outbox, view, total, n = capi.NodeOutbox(), capi.NodeAwait(), C.c_size_t(0), C.c_size_t(0)
    p = C.c_void_p()
    delivered = 0

    def ok(rc):
        assert rc == capi.OK, api.error()

    def rows(t):
        fresh["group"], fresh["block_id"], fresh["token"] = rng.integers(0, G, per_tick), 1, np.arange(per_tick) + (t + 1) * W
        return fresh

    def finish():  # the older step's outputs: its columns by view, its rows by view
        ok(api.node_outbox_view(h, C.byref(outbox)))
        ok(api.drain_applies_view(h, C.byref(p), C.byref(n)))
        ok(api.drain_messages_view(h, C.byref(p), C.byref(n)))

    times = []
    open_steps = 0
    for t in range(warmup + ticks):
        r = rows(t)
        t0 = time.perf_counter()
        now = 100 * (t + 1)
        if mode in ("awaited", "cancelled"):
            q = capi.NodeAwaitRequest(r.ctypes.data, len(r), 0, 0, now, len(out))
            if mode == "cancelled":
                keys = np.arange(16 * t, 16 * t + 16, dtype=np.uint64)  # (tokens of waiters that wait: registered at the start)
                q.cancel_keys, q.cancel_n, q.cancel_mask = keys.ctypes.data, 16, 2**64 - 1
            ok(api.step_node_awaited(h, now, flags, None, C.byref(q)))
        else:
            ok(api.step_node(h, now, flags))
        open_steps += 1
        if mode == "sync":
            finish()
            open_steps -= 1
            ok(api.engine_await_blocks(h, r.ctypes.data, len(r)))
            ok(api.engine_watch_completions(h, 0, now, out.ctypes.data, len(out), C.byref(total), None))
            delivered += min(total.value, len(out))
        elif open_steps == 2:
            finish()
            open_steps -= 1
            if mode in ("awaited", "cancelled"):
                ok(api.node_await_view(h, C.byref(view)))
                assert view.attached and view.marked == (16 if mode == "cancelled" else 0)
                delivered += view.rows_n
        times.append(time.perf_counter() - t0)
    while open_steps:
        finish()
        open_steps -= 1
        if mode in ("awaited", "cancelled"):
            ok(api.node_await_view(h, C.byref(view)))
            delivered += view.rows_n
    if mode != "plain":
        want = (warmup + ticks) * (per_tick + (16 if mode == "cancelled" else 0))
        assert delivered == want, (delivered, want)
    ms = np.array(times[warmup:]) * 1e3
    print(json.dumps(dict(mode=mode, slots=G, R=R, waiters=W, done_per_tick=per_tick if mode != "plain" else 0, ticks=ticks,
                          ms_per_tick_median=round(float(np.median(ms)), 3), q1=round(float(np.percentile(ms, 25)), 3),
                          q3=round(float(np.percentile(ms, 75)), 3), decisions_per_s=round(G / (float(np.median(ms)) * 1e-3), 0))))


if __name__ == "__main__":
    main(sys.argv[1], *[int(x) for x in sys.argv[2:3]])
