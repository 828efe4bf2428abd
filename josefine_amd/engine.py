"""Host-side mirror of josefine's Raft driver surface over the C ABI.

The reference drives one Raft group through

    trait Apply { fn apply(self, cmd: Command) -> Result<RaftHandle>; }
                                        (src/raft/mod.rs:483-489)

with `Command` (src/raft/mod.rs:160-227) as the input vocabulary and two
output channels, `rpc_tx` / `fsm_tx` (src/raft/mod.rs:337-340).  `BatchedRaft`
is the same surface for N groups at once: `Command` keeps the reference's
variant and field names, `RaftHandle` keeps `apply` / `is_leader` / … , and the
channels become `drain_messages()` / `drain_applies()`.

There is no CPU implementation behind this class: it binds
`josefine_amd/csrc/libjosefine_gpu.so` (HIP, gfx950) and raises if that
library is missing or no device is usable.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _capi as capi

_LIB_PATH = os.environ.get("JOSEFINE_GPU_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc",
                                                               "libjosefine_gpu.so")
_device_api: Optional[capi.Api] = None


class EngineError(RuntimeError):
    """A C-ABI call returned a negative status (anyhow::Error in the reference)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"josefine engine error {status}: {message}")
        self.status = status


def device_api() -> capi.Api:
    """Load the HIP engine library; never falls back to anything else."""
    global _device_api
    if _device_api is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(
                f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        api = capi.Api(_LIB_PATH, "jg_")
        # (tests/host_device.py compiles the engine for the host against an emulated runtime and marks that build: it is
        # test infrastructure, loaded by the tests' child processes only - never a way to run the product without a GPU)
        if hasattr(api.lib, "jg_emulated_device") and os.environ.get("JG_EMULATED_DEVICE") != "1":
            raise ImportError(f"{_LIB_PATH} is the tests' emulated-device build, not the gfx950 engine. There is no CPU fallback.")
        _device_api = api
    return _device_api


@dataclass
class Command:
    """enum Command (src/raft/mod.rs:160-227), flattened to the batch columns."""

    kind: int
    from_: int = 0
    term: int = 0
    id: int = 0
    aux: int = 0
    flag: int = 0
    blocks: List[Tuple[int, int]] = field(default_factory=list)  # Vec<Block> as (id, next)

    # constructors named after the reference variants and their fields
    @staticmethod
    def Tick() -> "Command":
        return Command(capi.CMD_TICK)

    @staticmethod
    def Propose() -> "Command":
        return Command(capi.CMD_PROPOSE)

    @staticmethod
    def VoteRequest(term: int, candidate_id: int, last_term: int, head: int) -> "Command":
        return Command(capi.CMD_VOTE_REQUEST, from_=candidate_id, term=term, id=head, aux=last_term)

    @staticmethod
    def VoteResponse(term: int, from_: int, granted: bool) -> "Command":
        return Command(capi.CMD_VOTE_RESPONSE, from_=from_, term=term, flag=int(granted))

    @staticmethod
    def AppendEntries(term: int, leader_id: int, blocks: Sequence[Tuple[int, int]]) -> "Command":
        return Command(capi.CMD_APPEND_ENTRIES, from_=leader_id, term=term, blocks=list(blocks))

    @staticmethod
    def AppendResponse(node_id: int, term: int, head: int, success: bool = True) -> "Command":
        return Command(capi.CMD_APPEND_RESPONSE, from_=node_id, term=term, id=head, flag=int(success))

    @staticmethod
    def Heartbeat(term: int, commit: int, leader_id: int) -> "Command":
        return Command(capi.CMD_HEARTBEAT, from_=leader_id, term=term, id=commit)

    @staticmethod
    def HeartbeatResponse(commit: int, has_committed: bool) -> "Command":
        return Command(capi.CMD_HEARTBEAT_RESPONSE, id=commit, flag=int(has_committed))

    @staticmethod
    def Timeout() -> "Command":
        return Command(capi.CMD_TIMEOUT)

    @staticmethod
    def Noop() -> "Command":
        return Command(capi.CMD_NOOP)

    @staticmethod
    def ClientRequest(id: int = 0) -> "Command":
        return Command(capi.CMD_CLIENT_REQUEST, id=id)

    @staticmethod
    def ClientResponse(id: int = 0) -> "Command":
        return Command(capi.CMD_CLIENT_RESPONSE, id=id)

    @staticmethod
    def Restart() -> "Command":
        """Engine op: process restart (Raft::new + Chain::new on the persisted tree)."""
        return Command(capi.CMD_RESTART)

    @staticmethod
    def Recreate() -> "Command":
        """Engine op: the replica of a partition that was re-created (Raft::new + Chain::new on an EMPTY directory)."""
        return Command(capi.CMD_RECREATE)


def expand_fsm_rows(rows: np.ndarray) -> np.ndarray:
    """FSM rows (capi.FSM_DTYPE) with every FSM_LEADER_STEP row (jg_step_node with JG_NODE_FSM_FUSED) replaced by the rows
    it stands for, in order: Apply {c0, c1} if c1 != c0, Notify {a, b}, Apply {c1, c2} if c2 != c1 (c_k = a - pad[k])."""
    rows = np.asarray(rows)
    fused = rows["kind"] == capi.FSM_LEADER_STEP
    if not fused.any():
        return rows
    a = rows["a"].astype(np.uint64)
    c = [a - rows["pad"][:, k].astype(np.uint64) for k in range(3)]
    pre, post = fused & (c[1] != c[0]), fused & (c[2] != c[1])
    count = np.where(fused, 1 + pre.astype(np.int64) + post.astype(np.int64), 1)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    out = np.zeros(int(count.sum()), dtype=rows.dtype)
    out[start[~fused]] = rows[~fused]
    i = np.nonzero(fused)[0]
    at = start[i]
    p = pre[i]
    out["group"][at[p]], out["kind"][at[p]], out["a"][at[p]], out["b"][at[p]] = rows["group"][i[p]], capi.FSM_APPLY_LEADER, c[0][i[p]], c[1][i[p]]
    at = at + p
    out["group"][at], out["kind"][at], out["a"][at], out["b"][at] = rows["group"][i], capi.FSM_NOTIFY, a[i], rows["b"][i]
    at = at + 1
    q = post[i]
    out["group"][at[q]], out["kind"][at[q]], out["a"][at[q]], out["b"][at[q]] = rows["group"][i[q]], capi.FSM_APPLY_LEADER, c[1][i[q]], c[2][i[q]]
    return out


def commit_rows_as_fsm(rows: np.ndarray) -> np.ndarray:
    """Rows of BatchedRaft.watch_commits (capi.COMMIT_ROW_DTYPE) as the FSM rows (capi.FSM_DTYPE) the dense entry points do
    not queue: every row that is CMT_COMMITTED and not CMT_REWOUND becomes FSM_APPLY_LEADER (where CMT_LEADS: keys
    (commit_from, commit]) or FSM_APPLY_FOLLOWER (keys [commit_from, commit)) {a = commit_from, b = commit}, in the rows'
    order.  A rewound row has no range: the consumer resynchronises its store from the row's commit / head."""
    rows = np.asarray(rows)
    st = rows["state"]
    r = rows[((st & capi.CMT_COMMITTED) != 0) & ((st & capi.CMT_REWOUND) == 0)]
    out = np.zeros(len(r), dtype=capi.FSM_DTYPE)
    out["group"], out["a"], out["b"] = r["group"], r["commit_from"], r["commit"]
    out["kind"] = np.where(r["state"] & capi.CMT_LEADS, capi.FSM_APPLY_LEADER, capi.FSM_APPLY_FOLLOWER)
    return out


class _Hosting:
    """Vacant slots (ABI v13): open_groups / close_groups / vacant_groups / hosted_groups over an engine handle (a
    BatchedRaft, or one shard of a multi-device one)."""

    def _group_set(self, groups, self_slots, device: bool, keep: list) -> "capi.GroupSet":
        s = capi.GroupSet()
        if isinstance(groups, range) and groups.step == 1 and self_slots is None and not device:
            s.g0, s.n = (groups.start, len(groups)) if len(groups) else (0, 0)
            return s
        g = np.asarray(list(groups) if not isinstance(groups, np.ndarray) else groups, dtype=np.int64).reshape(-1)
        order = np.argsort(g, kind="stable")
        g = g[order]
        if g.size and (g[0] < 0 or g[-1] >= (1 << 32)):
            raise EngineError(capi.EINVAL, "slot index out of range")
        if g.size > 1 and (np.diff(g) == 0).any():
            raise EngineError(capi.EINVAL, "a slot is listed twice")
        lst = np.ascontiguousarray(g, dtype=np.uint32)
        own = None
        if self_slots is not None:
            own = np.ascontiguousarray(np.asarray(self_slots, dtype=np.int64).reshape(-1)[order], dtype=np.uint8)
            assert own.shape == lst.shape, "one own slot per listed slot"
        s.n = lst.size
        if device:
            s.flags = capi.GROUPS_DEVICE
            for a, field in ((lst, "groups"), (own, "self_slots")):
                if a is None:
                    continue
                p = C.c_void_p()
                self._check(self.api.device_alloc(self._h, max(a.nbytes, 16), C.byref(p)))
                keep.append(p)
                if a.nbytes:
                    self._check(self.api.device_upload(self._h, p, a.ctypes.data, a.nbytes))
                setattr(s, field, p.value)
        else:
            keep += [lst, own]
            s.groups = lst.ctypes.data
            s.self_slots = own.ctypes.data if own is not None else None
        return s

    def _hosting_call(self, fn, groups, self_slots, device, *args) -> None:
        if hasattr(self, "_flush_pending"):
            self._flush_pending()
        keep: list = []
        try:
            s = self._group_set(groups, self_slots, device, keep)
            self._check(fn(self._h, *args, C.byref(s)))
        finally:
            for p in keep:
                if isinstance(p, C.c_void_p):
                    self.api.device_free(self._h, p)

    def open_groups(self, groups, now_ms: int = 0, self_slots=None, device: bool = False) -> None:
        """jg_engine_open_groups: every listed slot, which must be vacant, becomes what a JG_CMD_RECREATE row applied at
        now_ms makes of it.  `groups`: any iterable of slot indices (sorted here; a duplicate is refused) or a range;
        `self_slots`: the own replica slot per listed slot (in the order given); `device`: pass the list through this
        engine's device memory (JG_GROUPS_DEVICE)."""
        self._hosting_call(self.api.engine_open_groups, groups, self_slots, device, int(now_ms))

    def close_groups(self, groups, device: bool = False) -> None:
        """jg_engine_close_groups: every listed slot, which must host a partition, becomes vacant (the canonical record;
        the rows it produced before stay in the drains)."""
        self._hosting_call(self.api.engine_close_groups, groups, None, device)

    def _list(self, which: int, g0: int, n: Optional[int], limit: Optional[int]) -> np.ndarray:
        n = self.G - int(g0) if n is None else int(n)
        cap = n if limit is None else max(0, min(int(limit), n))
        out = np.zeros(max(cap, 1), np.uint32)
        total = C.c_size_t(0)
        self._check(self.api.engine_list_groups(self._h, which, int(g0), n, out.ctypes.data, cap, C.byref(total)))
        return out[:min(cap, total.value)]

    def vacant_groups(self, g0: int = 0, n: Optional[int] = None, limit: Optional[int] = None) -> np.ndarray:
        """jg_engine_list_groups(JG_LIST_VACANT): the vacant slots of g0 .. g0 + n - 1 ascending (the first `limit`)"""
        return self._list(capi.LIST_VACANT, g0, n, limit)

    def hosted_groups(self, g0: int = 0, n: Optional[int] = None, limit: Optional[int] = None) -> np.ndarray:
        """jg_engine_list_groups(JG_LIST_HOSTED): the slots of g0 .. g0 + n - 1 that host a partition, ascending"""
        return self._list(capi.LIST_HOSTED, g0, n, limit)

    def count_groups(self, vacant: bool = True, g0: int = 0, n: Optional[int] = None) -> int:
        """the number of vacant (or hosted) slots of g0 .. g0 + n - 1: jg_engine_list_groups with cap 0"""
        n = self.G - int(g0) if n is None else int(n)
        total = C.c_size_t(0)
        which = capi.LIST_VACANT if vacant else capi.LIST_HOSTED
        self._check(self.api.engine_list_groups(self._h, which, int(g0), n, None, 0, C.byref(total)))
        return int(total.value)


class BatchedRaft(_Hosting):
    """N independent Raft node instances behind one engine handle."""

    def __init__(self, n_groups: int, n_replicas: int = 1, node_ids: Optional[Sequence[int]] = None,
                 self_slots: Optional[Sequence[int]] = None, seed: int = 0, device_id: int = 0,
                 group_base: int = 0, flags: int = 0, heartbeat_timeout_ms: int = 100,
                 election_timeout_ms: Tuple[int, int] = (500, 1000), api: Optional[capi.Api] = None,
                 device_ids: Optional[Sequence[int]] = None, start_vacant: bool = False):
        """`device_ids` (HIP engine only): shard the groups over these devices behind this one
        handle (contiguous ownership; a device may be listed several times) — jg_config.n_devices.
        `start_vacant`: every slot starts vacant (JG_CFG_START_VACANT); open_groups makes partitions of them."""
        if start_vacant:
            flags |= capi.CFG_START_VACANT
        self.api = api if api is not None else device_api()
        self.G, self.R = int(n_groups), int(n_replicas)
        if node_ids is None:
            node_ids = list(range(1, self.R + 1))  # examples/multi-node/node-*.toml: ids 1..R
        cfg = capi.Config()
        cfg.abi_version = capi.ABI_VERSION
        cfg.n_groups = self.G
        cfg.n_replicas = self.R
        for r, nid in enumerate(list(node_ids)[:capi.MAX_REPLICAS]):
            cfg.node_ids[r] = int(nid)
        cfg.device_id = device_id
        if device_ids is not None:
            assert 1 <= len(device_ids) <= capi.MAX_DEVICES
            cfg.n_devices = len(device_ids)
            for d, dev in enumerate(device_ids):
                cfg.device_ids[d] = int(dev)
        cfg.heartbeat_timeout_ms = heartbeat_timeout_ms
        cfg.election_timeout_min_ms, cfg.election_timeout_max_ms = election_timeout_ms
        cfg.seed = seed
        cfg.group_base = group_base
        cfg.flags = flags
        self.node_ids = [int(x) for x in node_ids]
        self.cfg = cfg
        h = C.c_void_p()
        self._check(self.api.engine_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._pending: List[Tuple[int, Command]] = []
        if self_slots is not None:
            s = np.ascontiguousarray(self_slots, dtype=np.uint8)
            assert s.shape == (self.G,)
            self._check(self.api.set_self_slots(self._h, s.ctypes.data))

    # -- lifecycle -----------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self.api.engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status: int) -> None:
        if status != capi.OK:
            raise EngineError(status, self.api.error())

    # -- shards of a multi-device engine -------------------------------------
    @property
    def n_shards(self) -> int:
        return int(self.api.shard_count(self._h)) if hasattr(self.api, "shard_count") else 1

    def shard(self, d: int) -> "Shard":
        """Shard d's own single-device engine (jg_get_shard): what the device-pointer entry
        points are called on."""
        info = capi.ShardInfo()
        self._check(self.api.get_shard(self._h, d, C.byref(info)))
        return Shard(self, info)

    def step_dense_acks_shards(self, ptrs: Sequence[int], n_ticks: int = 1) -> None:
        """jg_step_dense_acks_shards: ptrs[d] = shard d's device-resident [n_ticks][R][G_d] block."""
        arr = (C.c_void_p * len(ptrs))(*[C.c_void_p(int(p)) for p in ptrs])
        self._check(self.api.step_dense_acks_shards(self._h, arr, int(n_ticks)))

    # -- input ---------------------------------------------------------------
    def submit(self, group: int, cmd: Command) -> None:
        """Queue `cmd` for `group`; applied at the next step() in submit order."""
        self._pending.append((int(group), cmd))

    def submit_columns(self, kind, group, from_=None, term=None, id=None, aux=None, flag=None,
                       blk_id=None, blk_next=None) -> None:
        """Queue a whole SoA batch (numpy columns) — jg_submit as is."""
        self._flush_pending()
        n = len(kind)

        def col(x, dt):
            if x is None:
                return None  # an absent column: all zeros, and not even uploaded by jg_step_node
            return np.ascontiguousarray(x, dtype=dt)

        cols = [col(kind, np.uint8), col(group, np.uint32), col(from_, np.uint32), col(term, np.uint64),
                col(id, np.uint64), col(aux, np.uint64), col(flag, np.uint8)]
        bi = np.ascontiguousarray(blk_id if blk_id is not None else [], dtype=np.uint64)
        bn = np.ascontiguousarray(blk_next if blk_next is not None else [], dtype=np.uint64)
        b = capi.CmdBatch()
        b.n = n
        (b.kind, b.group, b.from_, b.term, b.id, b.aux, b.flag) = [None if c is None else c.ctypes.data for c in cols]
        b.n_blocks = len(bi)
        b.blk_id, b.blk_next = bi.ctypes.data, bn.ctypes.data
        self._check(self.api.submit(self._h, C.byref(b)))

    def _flush_pending(self) -> None:
        if not self._pending:
            return
        pend, self._pending = self._pending, []
        n = len(pend)
        kind = np.zeros(n, np.uint8)
        group = np.zeros(n, np.uint32)
        from_ = np.zeros(n, np.uint32)
        term = np.zeros(n, np.uint64)
        id_ = np.zeros(n, np.uint64)
        aux = np.zeros(n, np.uint64)
        flag = np.zeros(n, np.uint8)
        bi: List[int] = []
        bn: List[int] = []
        for i, (g, c) in enumerate(pend):
            kind[i], group[i], from_[i], term[i], flag[i] = c.kind, g, c.from_, c.term, c.flag
            if c.kind == capi.CMD_APPEND_ENTRIES:
                id_[i], aux[i] = len(bi), len(c.blocks)
                for (b_id, b_next) in c.blocks:
                    bi.append(b_id)
                    bn.append(b_next)
            else:
                id_[i], aux[i] = c.id, c.aux
        self.submit_columns(kind, group, from_, term, id_, aux, flag, bi, bn)

    def step(self, now_ms: int = 0) -> None:
        """Apply everything submitted, per group in stream order (Apply::apply)."""
        self._flush_pending()
        self._check(self.api.step(self._h, int(now_ms)))

    def apply(self, group: int, cmd: Command, now_ms: int = 0) -> "RaftHandle":
        """RaftHandle::apply for one group: submit + step."""
        self.submit(group, cmd)
        self.step(now_ms)
        return RaftHandle(self, group)

    def apply_all(self, cmd: Command, now_ms: int = 0) -> None:
        """Apply the same command to every group."""
        n = self.G
        self.submit_columns(np.full(n, cmd.kind, np.uint8), np.arange(n, dtype=np.uint32),
                            np.full(n, cmd.from_, np.uint32), np.full(n, cmd.term, np.uint64),
                            np.full(n, cmd.id, np.uint64), np.full(n, cmd.aux, np.uint64),
                            np.full(n, cmd.flag, np.uint8))
        self.step(now_ms)

    def step_dense_acks(self, acks: np.ndarray) -> None:
        """Dense leader tick from a host [R, G] uint64 array (jg_step_dense_acks)."""
        self._flush_pending()
        a = np.ascontiguousarray(acks, dtype=np.uint64)
        assert a.shape == (self.R, self.G), a.shape
        self._check(self.api.step_dense_acks(self._h, a.ctypes.data))

    def step_node(self, now_ms: int = 0, leader: bool = True, follower: bool = True, tick: bool = True, async_: bool = False,
                  between=None, common_ae: bool = False, fsm_fused: bool = False) -> dict:
        """jg_step_node: a node's whole tick from the rows submitted since the last step - rows in the
        mailbox vocabulary through the dense kernels, everything else through the general state
        machine first - then Command::Tick for every partition.  Returns the outbox columns (host
        copies): beat_term / beat_commit [G], ae [R, G] words, answer / hb_commit [G], and the step's
        row / PCIe byte counts.  common_ae (JG_NODE_COMMON_AE): "aec" [G] is the partition's AppendEntries word
        for every addressee, "ae" only comes down (else None) when some partition's words differ (AEC_INDIVIDUAL);
        fsm_fused (JG_NODE_FSM_FUSED): a leader's rows of a step as one FSM_LEADER_STEP row (`expand_fsm_rows`)."""
        self.step_node_begin(now_ms, leader, follower, tick, async_, common_ae, fsm_fused)
        if between is not None:  # (async_: what the caller does while the step runs - submits for the next one, say)
            between()
        return self.node_outbox()

    def step_node_begin(self, now_ms: int = 0, leader: bool = True, follower: bool = True, tick: bool = True, async_: bool = False,
                        common_ae: bool = False, fsm_fused: bool = False, keep: bool = False, poll: Optional[dict] = None,
                        completions: Optional[dict] = None, lookup: Optional[dict] = None, hosting: Optional[dict] = None) -> None:
        """jg_step_node alone (the outbox: `node_outbox`).  keep (JG_NODE_KEEP, with async_): the step keeps its outputs
        until its outbox is viewed - a second such step may be begun before that; `node_outbox` then serves the OLDER
        one and makes its rows the ones the next drains deliver.  poll (jg_step_node_polled, ABI v21; with keep): the
        keyword arguments of `poll` as a dict - the poll travels with the step, sees the engine exactly as the step leaves
        it and is handed out by `node_poll` once the step's outbox has been viewed.  completions (jg_step_node_awaited,
        ABI v23; with keep): dict(groups=, block_ids=, tokens=, terms=0, deadlines_ms=0, now_ms=, limit=None, peek=False,
        stats=False, cancel_keys=(), cancel_mask=2**64 - 1) - the waiters of `await_blocks` (optional: without them the
        step only watches) are registered, the cancel of `cancel_waiters` (ABI v24; optional) is made and the watch of
        `watch_completions` is made behind the step; `node_completions` hands out the answer.  lookup (jg_step_node_looked,
        ABI v25; with keep): dict(groups=None, g0=0, n=None, progress=False), the arguments of `lookup` - the point query is
        made behind the step, on the engine exactly as the step leaves it; `node_lookup` hands out the answer.  hosting
        (jg_step_node_hosted, ABI v26; with keep): dict(close=None, open=None, self_slots=None) - `close` and `open` as the
        `groups` of `close_groups` and `open_groups` (an iterable of slot indices or a range), `self_slots` the open's own
        slots: behind everything else of the step the engine becomes what close_groups(close) and then
        open_groups(open, now_ms, self_slots) make of it; `node_hosting` hands out the verdict."""
        self._flush_pending()
        flags = (capi.NODE_LEADER_HALF if leader else 0) | (capi.NODE_FOLLOWER_HALF if follower else 0) | \
                (capi.NODE_TICK if tick else 0) | (capi.NODE_ASYNC if async_ else 0) | \
                (capi.NODE_COMMON_AE if common_ae else 0) | (capi.NODE_FSM_FUSED if fsm_fused else 0) | \
                (capi.NODE_KEEP if keep else 0)
        if lookup is not None or hosting is not None:
            entry = "step_node_looked" if hosting is None else "step_node_hosted"
            if not hasattr(self.api, entry):
                raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}{entry}")
            p = held = req = rows = s = lst = None
            if poll is not None:
                p, held, parts = self._poll_request(**poll)
            if completions is not None:
                req, rows, want_stats = self._await_request(**completions)
            if lookup is not None:
                s, lst = self._lookup_set(**lookup)  # (`lst`: what s points at, alive over the call)
            args = (self._h, int(now_ms), flags, C.byref(p) if p is not None else None, C.byref(req) if req is not None else None,
                    C.byref(s) if s is not None else None)
            if hosting is None:
                self._check(self.api.step_node_looked(*args))
            else:
                hr, sets = self._hosting_request(**hosting)  # (`sets`: what hr points at, alive over the call)
                self._check(self.api.step_node_hosted(*args, C.byref(hr)))
                del sets
            del held, lst
            if completions is not None:
                self._await_n = getattr(self, "_await_n", 0) + len(rows)
        elif completions is not None:
            if not hasattr(self.api, "step_node_awaited"):
                raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}step_node_awaited")
            p = held = None
            if poll is not None:
                p, held, parts = self._poll_request(**poll)
            req, rows, want_stats = self._await_request(**completions)  # (`rows`, req.held: what req points at, alive over the call)
            self._check(self.api.step_node_awaited(self._h, int(now_ms), flags, C.byref(p) if p is not None else None, C.byref(req)))
            del held
            self._await_n = getattr(self, "_await_n", 0) + len(rows)  # (the bound: what the views take off it is not known yet)
        elif poll is not None:
            if not hasattr(self.api, "step_node_polled"):
                raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}step_node_polled")
            p, held, parts = self._poll_request(**poll)  # (`held`: what p points at, alive over the call)
            self._check(self.api.step_node_polled(self._h, int(now_ms), flags, C.byref(p)))
            del held
        else:
            self._check(self.api.step_node(self._h, int(now_ms), flags))
        if keep:  # (what node_poll needs to know of the step and the view does not say: was the backlog asked for)
            self.__dict__.setdefault("_kept_backlog", []).append(bool(poll is not None and parts["backlog"]))
            # (... and what node_completions needs: were the stats asked for, does the watch remove what it delivers)
            self.__dict__.setdefault("_kept_await", []).append(
                None if completions is None else (want_stats, not completions.get("peek", False)))

    def _await_request(self, groups=(), block_ids=(), tokens=(), terms=0, deadlines_ms=0, now_ms: int = 0, limit: Optional[int] = None,
                       peek: bool = False, stats: bool = False, cancel_keys=(), cancel_mask: int = 2**64 - 1):
        """jg_node_await_request from the keyword arguments of `await_blocks` and `watch_completions`"""
        groups = np.atleast_1d(np.asarray(groups))
        rows = np.zeros(len(groups), capi.AWAIT_ROW_DTYPE)
        if len(groups) and (groups.min() < 0 or groups.max() > 0xFFFFFFFF):
            raise EngineError(capi.EINVAL, "completions: group out of range")
        rows["group"] = groups
        for name, v in (("block_id", block_ids), ("token", tokens), ("term", terms), ("deadline_ms", deadlines_ms)):
            rows[name] = np.asarray(v, dtype=np.uint64)
        have = getattr(self, "_await_n", 0) + len(rows)
        req = capi.NodeAwaitRequest()
        req.rows, req.n = rows.ctypes.data if len(rows) else None, len(rows)
        req.flags, req.want_stats, req.now_ms = capi.WATCH_PEEK if peek else 0, 1 if stats else 0, int(now_ms)
        req.cap = have if limit is None else max(0, min(int(limit), have))
        keys = np.ascontiguousarray(np.atleast_1d(np.asarray(cancel_keys, dtype=np.uint64)))
        if len(keys):
            req.cancel_keys, req.cancel_n, req.cancel_mask = keys.ctypes.data, len(keys), int(cancel_mask)
            req.held = keys
        return req, rows, bool(stats)

    def node_completions(self):
        """jg_node_await_view: the answer of the completion request that travelled with the kept step whose outbox
        `node_outbox` viewed last, as host copies: {"answer": what `watch_completions` returns for the same arguments -
        (rows, total) or (rows, total, stats) - "marked": the waiters the step's cancel newly marked (what `cancel_waiters`
        returns), and "redone": the step had general-path rows and the chain ran behind its catch-up pass
        (informational)}.  A step that carried no request: {"redone": False}."""
        if not hasattr(self.api, "node_await_view"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}node_await_view")
        v = capi.NodeAwait()
        self._check(self.api.node_await_view(self._h, C.byref(v)))
        if not v.attached:
            return {"redone": False}
        k = int(v.rows_n)
        rows = np.zeros(0, capi.DONE_ROW_DTYPE)
        if k:
            buf = (C.c_char * (k * np.dtype(capi.DONE_ROW_DTYPE).itemsize)).from_address(v.rows)
            rows = np.frombuffer(buf, dtype=capi.DONE_ROW_DTYPE).copy()
        out = (rows, int(v.total))
        if self.__dict__.get("_viewed_await_stats", False):
            out += ({name: int(getattr(v.stats, name)) for name, _ in capi.AwaitStats._fields_},)
        return {"answer": out, "marked": int(v.marked), "redone": bool(v.state & capi.NODE_POLL_REDONE)}

    def _view_await(self):
        """behind a view of a kept step's outbox: the waiters its completion request removed leave the count that
        `watch_completions` sizes its rows from"""
        self._viewed_await_stats = False
        kept = self.__dict__.get("_kept_await")
        what = kept.pop(0) if kept else None
        if what is None:
            return
        self._viewed_await_stats, removes = what
        v = capi.NodeAwait()
        self._check(self.api.node_await_view(self._h, C.byref(v)))
        if removes:
            self._await_n = getattr(self, "_await_n", 0) - int(v.rows_n)

    def node_poll(self) -> dict:
        """jg_node_poll_view: the answer of the poll that travelled with the kept step whose outbox `node_outbox` viewed
        last, as host copies - the dict `poll` returns for the same arguments (every part the step's request named), plus
        "redone": the step had general-path rows and the poll ran once more behind its catch-up pass (informational).  A
        step that carried no poll: {"redone": False}."""
        if not hasattr(self.api, "node_poll_view"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}node_poll_view")
        v = capi.NodePoll()
        self._check(self.api.node_poll_view(self._h, C.byref(v)))

        def rows(p, k, dtype):
            k = int(k)
            if not k:
                return np.zeros(0, dtype)
            buf = (C.c_char * (k * np.dtype(dtype).itemsize)).from_address(p)
            return np.frombuffer(buf, dtype=dtype).copy()

        out = {}
        if v.want & capi.POLL_LEADERS:
            out["leaders"] = rows(v.leaders, v.leaders_n, capi.LEADER_ROW_DTYPE), int(v.leaders_total)
        if v.want & capi.POLL_REPLICAS:
            out["replicas"] = rows(v.replicas, v.replicas_n, capi.ISR_ROW_DTYPE), int(v.replicas_total)
        if v.want & capi.POLL_COMMITS:
            out["commits"] = rows(v.commits, v.commits_n, capi.COMMIT_ROW_DTYPE), int(v.commits_total)
            if self.__dict__.get("_viewed_backlog", False):
                out["commits"] += ({name: int(getattr(v.backlog, name)) for name, _ in capi.CommitBacklog._fields_},)
        if v.want & capi.POLL_CENSUS:
            out["census"] = self._census_dict(v.census)
        if v.want & capi.POLL_REPL_CENSUS:
            out["repl_census"] = self._repl_census_dict(v.repl_census)
        out["redone"] = bool(v.state & capi.NODE_POLL_REDONE)
        return out

    def node_outbox(self) -> dict:
        """jg_node_outbox_view as host copies (see `step_node`)."""
        o = capi.NodeOutbox()
        self._check(self.api.node_outbox_view(self._h, C.byref(o)))
        if self.__dict__.get("_kept_backlog"):  # (kept steps were outstanding: the view served the oldest)
            self._viewed_backlog = self._kept_backlog.pop(0)
            self._view_await()
        G, R = self.G, self.R

        def arr(p, dt, shape):
            if not p:
                return None
            n = int(np.prod(shape))
            buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(p)
            return np.frombuffer(buf, dtype=dt).reshape(shape).copy()

        beat = arr(o.beat, np.dtype([("term", "<u8"), ("hb_commit", "<u8")]), (G,))
        return {"beat_term": None if beat is None else beat["term"].copy(),
                "beat_commit": None if beat is None else beat["hb_commit"].copy(),
                "ae": arr(o.ae, np.uint64, (R, G)), "aec": arr(o.aec, np.uint64, (G,)), "answer": arr(o.answer, np.uint64, (G,)),
                "hb_commit": arr(o.hb_commit, np.uint64, (G,)), "rows": int(o.rows), "rows_general": int(o.rows_general),
                "bytes_h2d": int(o.bytes_h2d), "bytes_d2h": int(o.bytes_d2h)}

    def node_inbox_columns(self, slot: int, answer, hb_commit=None) -> None:
        """jg_node_inbox_columns: member slot `slot`'s AppendResponse / HeartbeatResponse for every partition
        as ONE column of JG_ANSWER words (and, optionally, the HeartbeatResponse.commit column) for the next
        step_node - what a batched peer ships instead of two rows per partition."""
        pa, ph = C.c_void_p(), C.c_void_p()
        self._check(self.api.node_inbox_columns(self._h, int(slot), C.byref(pa), C.byref(ph) if hb_commit is not None else None))
        G = self.G
        np.frombuffer((C.c_char * (8 * G)).from_address(pa.value), dtype=np.uint64)[:] = np.asarray(answer, dtype=np.uint64)
        if hb_commit is not None:
            np.frombuffer((C.c_char * (8 * G)).from_address(ph.value), dtype=np.uint64)[:] = np.asarray(hb_commit, dtype=np.uint64)

    def upload_rows(self, kind, group, from_=None, term=None, id=None, aux=None, flag=None,
                    blk_id=None, blk_next=None) -> "DeviceRows":
        """Sort a command batch by group (stable) on the host and park it in device memory for
        step_device_rows — how a caller keeps a pre-built trace resident in HBM."""
        n = len(kind)
        order = np.argsort(np.asarray(group, dtype=np.uint32), kind="stable")

        def col(x, dt):
            a = np.zeros(n, dtype=dt) if x is None else np.asarray(x, dtype=dt)
            return np.ascontiguousarray(a[order])

        cols = [col(kind, np.uint8), col(group, np.uint32), col(from_, np.uint32), col(term, np.uint64),
                col(id, np.uint64), col(aux, np.uint64), col(flag, np.uint8)]
        side = [np.ascontiguousarray(x if x is not None else [], dtype=np.uint64) for x in (blk_id, blk_next)]
        return DeviceRows(self, cols, side)

    def upload_u32(self, values) -> "DeviceList":
        """A list of uint32 (group numbers) parked in device memory: jg_dense_cluster_withdraw_appends / _offer_appends."""
        return DeviceList(self, np.ascontiguousarray(values, dtype=np.uint32))

    def step_device_rows(self, rows: "DeviceRows", now_ms: int = 0) -> None:
        """jg_step_device_rows: apply a device-resident, group-sorted batch (no host pass)."""
        self._flush_pending()
        self._check(self.api.step_device_rows(self._h, C.byref(rows.batch), int(now_ms)))

    def step_dense_acks_n(self, acks: np.ndarray) -> None:
        """T consecutive dense ticks from a host [T, R, G] array.  On the device engine this is
        ONE launch (jg_step_dense_acks_device_n: state read and written once); a backend without
        that entry point gets the T ticks one by one — the two are specified to be identical."""
        self._flush_pending()
        a = np.ascontiguousarray(acks, dtype=np.uint64)
        assert a.ndim == 3 and a.shape[1:] == (self.R, self.G), a.shape
        if not hasattr(self.api, "step_dense_acks_device_n"):
            for t in range(a.shape[0]):
                self._check(self.api.step_dense_acks(self._h, a[t].ctypes.data))
            return
        buf = C.c_void_p()
        self._check(self.api.device_alloc(self._h, a.nbytes, C.byref(buf)))
        try:
            self._check(self.api.device_upload(self._h, buf, a.ctypes.data, a.nbytes))
            self._check(self.api.step_dense_acks_device_n(self._h, buf, a.shape[0]))
            self._check(self.api.sync(self._h))
        finally:
            self.api.device_free(self._h, buf)

    # -- dense node tick (host-array convenience over the device-pointer ABI) ---------------
    def _is_device(self) -> bool:
        return hasattr(self.api, "device_alloc")

    def _to_engine(self, arr: Optional[np.ndarray], keep: list):
        """Host array -> pointer the engine accepts (device copy for the HIP engine)."""
        if arr is None:
            return None
        a = np.ascontiguousarray(arr)
        if not self._is_device():
            keep.append(a)
            return a.ctypes.data
        p = C.c_void_p()
        self._check(self.api.device_alloc(self._h, max(a.nbytes, 16), C.byref(p)))
        self._check(self.api.device_upload(self._h, p, a.ctypes.data, a.nbytes))
        keep.append(p)
        return p.value

    def _out_buffer(self, shape, dtype, keep: list):
        host = np.zeros(shape, dtype=dtype)
        if not self._is_device():
            keep.append(host)
            return host, host.ctypes.data
        p = C.c_void_p()
        self._check(self.api.device_alloc(self._h, max(host.nbytes, 16), C.byref(p)))
        keep.append(p)
        return host, p.value

    def _finish(self, outs, keep) -> None:
        if self._is_device():
            for host, ptr in outs:
                self._check(self.api.device_download(self._h, host.ctypes.data, C.c_void_p(ptr), host.nbytes))
            for k in keep:
                if isinstance(k, C.c_void_p):
                    self.api.device_free(self._h, k)

    def step_dense_leader(self, now_ms: int = 0, acks: Optional[np.ndarray] = None,
                          hbr_has: Optional[np.ndarray] = None, hbr_commit: Optional[np.ndarray] = None,
                          tick: bool = True) -> Optional[dict]:
        """Leader half of a node tick (jg_step_dense_leader) over host arrays in column form: the
        AppendResponse heads (own slot: #appends) and HeartbeatResponse codes are packed into the
        inbox's answer words here, the outbox words are unpacked into {term, hb_commit, ae_from,
        ae_n}; returns None when `tick` is false."""
        assert not self._pending
        keep: list = []
        inbox = capi.LeaderInbox()
        if acks is not None or hbr_has is not None:
            a = np.full((self.R, self.G), capi.NO_ACK, np.uint64) if acks is None else \
                np.asarray(acks, np.uint64).reshape(self.R, self.G)
            if acks is None:  # only HeartbeatResponses: nobody appends
                a[self.read("self_slot"), np.arange(self.G)] = 0
            h = np.full((self.R, self.G), capi.HB_NONE, np.uint8) if hbr_has is None else \
                np.asarray(hbr_has, np.uint8).reshape(self.R, self.G)
            c = np.zeros((self.R, self.G), np.uint64) if hbr_commit is None else \
                np.asarray(hbr_commit, np.uint64).reshape(self.R, self.G)
            inbox.answers = self._to_engine(np.ascontiguousarray(capi.pack_answers(a, h)), keep)
            inbox.hbr_commit = self._to_engine(c, keep)
        outs, res = [], None
        outbox_p = None
        if tick:
            outbox = capi.LeaderOutbox()
            beat, outbox.beat = self._out_buffer((self.G, 2), np.uint64, keep)
            ae, outbox.ae = self._out_buffer((self.R, self.G), np.uint64, keep)
            # (row [own slot] of the block is nobody's mail and is not written while the own slot is the same for
            # every group: JG_NO_ACK by the block's owner, include/josefine_gpu.h jg_leader_outbox)
            ae[:] = np.uint64(capi.NO_ACK)
            if self._is_device():
                self._check(self.api.device_upload(self._h, C.c_void_p(outbox.ae), ae.ctypes.data, ae.nbytes))
            outs = [(beat, outbox.beat), (ae, outbox.ae)]
            outbox_p = C.byref(outbox)
        try:
            self._check(self.api.step_dense_leader(self._h, now_ms, C.byref(inbox), outbox_p))
        finally:
            self._finish(outs, keep)
        if tick:
            ae_from, ae_n = capi.unpack_ae(ae)
            res = {"term": np.ascontiguousarray(beat[:, 0]), "hb_commit": np.ascontiguousarray(beat[:, 1]),
                   "ae_from": ae_from, "ae_n": ae_n}
        return res

    def step_dense_follower(self, now_ms: int, term, hb_commit, ae_from, ae_n, leader=None, leader_id: int = 0,
                            tick: bool = True) -> dict:
        """Follower half of a node tick (jg_step_dense_follower) over host arrays in column form
        (packed into the inbox words here); returns the answers unpacked: {ack_head, hb_commit, hb_has}."""
        assert not self._pending
        keep: list = []
        inbox = capi.FollowerInbox()
        inbox.leader = self._to_engine(None if leader is None else np.asarray(leader, np.uint32), keep)
        inbox.leader_id = int(leader_id)
        beat = np.stack([np.asarray(term, np.uint64), np.asarray(hb_commit, np.uint64)], axis=1)
        inbox.beat = self._to_engine(np.ascontiguousarray(beat), keep)
        inbox.ae = self._to_engine(np.ascontiguousarray(capi.pack_ae(ae_from, ae_n)), keep)
        outbox = capi.FollowerOutbox()
        answer, outbox.answer = self._out_buffer((self.G,), np.uint64, keep)
        hbc, outbox.hb_commit = self._out_buffer((self.G,), np.uint64, keep)
        outs = [(answer, outbox.answer), (hbc, outbox.hb_commit)]
        try:
            self._check(self.api.step_dense_follower(self._h, now_ms, C.byref(inbox), C.byref(outbox), 1 if tick else 0))
        finally:
            self._finish(outs, keep)
        ack_head, hb_has = capi.unpack_answers(answer)
        return {"ack_head": ack_head, "hb_commit": np.where(hb_has != capi.HB_NONE, hbc, np.uint64(0)), "hb_has": hb_has}

    # -- output --------------------------------------------------------------
    def _drain(self, fn, dtype) -> np.ndarray:
        n = C.c_size_t(0)
        self._check(fn(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=dtype)
        if n.value:
            self._check(fn(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def _drain_view(self, fn, dtype, copy: bool) -> np.ndarray:
        """One call: the rows sit in the engine's pinned host queue; `copy=False` returns a
        numpy view of it that is valid until the engine's next synchronising call."""
        p, n = C.c_void_p(), C.c_size_t(0)
        self._check(fn(self._h, C.byref(p), C.byref(n)))
        dt = np.dtype(dtype)
        if not n.value:
            return np.zeros(0, dtype=dt)
        buf = (C.c_char * (n.value * dt.itemsize)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dt)
        return arr.copy() if copy else arr

    def drain_messages(self, copy: bool = True) -> np.ndarray:
        """Everything the groups pushed on rpc_tx since the last drain."""
        if hasattr(self.api, "drain_messages_view"):
            return self._drain_view(self.api.drain_messages_view, capi.MSG_DTYPE, copy)
        return self._drain(self.api.drain_messages, capi.MSG_DTYPE)

    def drain_applies(self, copy: bool = True) -> np.ndarray:
        """Everything the groups pushed on fsm_tx since the last drain."""
        if hasattr(self.api, "drain_applies_view"):
            return self._drain_view(self.api.drain_applies_view, capi.FSM_DTYPE, copy)
        return self._drain(self.api.drain_applies, capi.FSM_DTYPE)

    def drain_prefetch(self) -> None:
        """jg_drain_prefetch: start moving everything stepped so far to the host queues without
        blocking (a no-op while the previous batch is still in transfer); from now on the drains
        deliver what has landed and never block."""
        self._flush_pending()
        self._check(self.api.drain_prefetch(self._h))

    def drain_wait(self) -> None:
        """jg_drain_wait: block until the batch in transfer (if any) has landed."""
        self._check(self.api.drain_wait(self._h))

    def drain_flush(self) -> None:
        """jg_drain_flush: block until everything stepped so far has landed in the host queues."""
        self._flush_pending()
        self._check(self.api.drain_flush(self._h))

    def drain_faults(self) -> np.ndarray:
        return self._drain(self.api.drain_faults, capi.FAULT_DTYPE)

    def read(self, field_name: str, replica: int = 0, g0: int = 0, n: Optional[int] = None) -> np.ndarray:
        fld = capi.FIELD_NAMES[field_name]
        n = self.G - g0 if n is None else n
        out = np.zeros(n, dtype=capi.FIELD_DTYPES[fld])
        if n:
            self._check(self.api.read_state(self._h, fld, replica, out.ctypes.data, g0, n))
        return out

    def watch_leaders(self, g0: int = 0, n: Optional[int] = None, limit: Optional[int] = None, peek: bool = False):
        """jg_engine_watch_leaders: the slots of g0 .. g0 + n - 1 whose leadership view (role, term, known leader, fault,
        vacancy) differs from what this feed last reported, ascending, as their current view: (rows, total) with rows a
        structured array (capi.LEADER_ROW_DTYPE) of the first `limit` of them and total their number.  The delivered
        slots become "seen"; `peek` delivers the same rows and advances nothing.  One feed per engine."""
        n = self.G - int(g0) if n is None else int(n)
        if not hasattr(self.api, "engine_watch_leaders"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_watch_leaders")
        cap = n if limit is None else max(0, min(int(limit), n))
        out = np.zeros(max(cap, 1), capi.LEADER_ROW_DTYPE)
        total = C.c_size_t(0)
        flags = capi.WATCH_PEEK if peek else 0
        self._check(self.api.engine_watch_leaders(self._h, flags, int(g0), n, out.ctypes.data, cap, C.byref(total)))
        return out[:min(cap, total.value)], int(total.value)

    def census(self, g0: int = 0, n: Optional[int] = None) -> dict:
        """jg_engine_census over the slots g0 .. g0 + n - 1: a dict of jg_census's fields (led_by: a list of R counts,
        one per member of node_ids)."""
        n = self.G - int(g0) if n is None else int(n)
        if not hasattr(self.api, "engine_census"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_census")
        c = capi.Census()
        self._check(self.api.engine_census(self._h, int(g0), n, C.byref(c)))
        out = {name: int(getattr(c, name)) for name, t in capi.Census._fields_ if name != "led_by"}
        out["led_by"] = [int(x) for x in c.led_by[:self.R]]
        return out

    def watch_replicas(self, leave_lag: int, join_lag: Optional[int] = None, g0: int = 0, n: Optional[int] = None,
                       limit: Optional[int] = None, peek: bool = False):
        """jg_engine_watch_replicas: the slots of g0 .. g0 + n - 1 whose in-sync set (or whether the slot leads at all)
        differs from what this feed last reported, ascending, as their current view: (rows, total) with rows a structured
        array (capi.ISR_ROW_DTYPE) of the first `limit` of them and total their number.  A member the feed last reported
        in sync stays while its lag is <= leave_lag, any other joins at lag <= join_lag (default: leave_lag).  The delivered
        slots become "seen"; `peek` delivers the same rows and advances nothing.  One feed per engine."""
        n = self.G - int(g0) if n is None else int(n)
        if not hasattr(self.api, "engine_watch_replicas"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_watch_replicas")
        cap = n if limit is None else max(0, min(int(limit), n))
        out = np.zeros(max(cap, 1), capi.ISR_ROW_DTYPE)
        total = C.c_size_t(0)
        pol = capi.IsrPolicy(int(leave_lag), int(leave_lag if join_lag is None else join_lag))
        flags = capi.WATCH_PEEK if peek else 0
        self._check(self.api.engine_watch_replicas(self._h, flags, C.byref(pol), int(g0), n, out.ctypes.data, cap, C.byref(total)))
        return out[:min(cap, total.value)], int(total.value)

    def watch_replicas_timed(self, now_ms: int, max_behind_ms: int, caught_lag: int = 0, join_lag: int = 0, g0: int = 0,
                             n: Optional[int] = None, limit: Optional[int] = None, peek: bool = False):
        """jg_engine_watch_replicas_timed: watch_replicas under the time rule (replica.lag.time.max.ms) - the same feed, the
        same rows and the same shadow, (rows, total).  A member the feed last reported in sync stays until it has been behind
        (lag > caught_lag) for more than max_behind_ms of the caller's clock, sampled at the calls; any other joins at lag <=
        join_lag (<= caught_lag).  Unless `peek`, the clocks of EVERY slot of the range advance to now_ms, delivered or not,
        and the delivered slots become "seen"; `peek` delivers the same rows and advances neither."""
        n = self.G - int(g0) if n is None else int(n)
        if not hasattr(self.api, "engine_watch_replicas_timed"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_watch_replicas_timed")
        cap = n if limit is None else max(0, min(int(limit), n))
        out = np.zeros(max(cap, 1), capi.ISR_ROW_DTYPE)
        total = C.c_size_t(0)
        clk = capi.IsrClock(int(now_ms), int(max_behind_ms), int(caught_lag), int(join_lag))
        flags = capi.WATCH_PEEK if peek else 0
        self._check(self.api.engine_watch_replicas_timed(self._h, flags, C.byref(clk), int(g0), n, out.ctypes.data, cap, C.byref(total)))
        return out[:min(cap, total.value)], int(total.value)

    def replication_census(self, lag_limit: int, g0: int = 0, n: Optional[int] = None) -> dict:
        """jg_engine_replication_census over the slots g0 .. g0 + n - 1 with the one threshold lag_limit: a dict of
        jg_repl_census's fields (out_of_sync / max_lag / sum_lag: lists of R values, one per member slot)."""
        n = self.G - int(g0) if n is None else int(n)
        if not hasattr(self.api, "engine_replication_census"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_replication_census")
        c = capi.ReplCensus()
        self._check(self.api.engine_replication_census(self._h, int(lag_limit), int(g0), n, C.byref(c)))
        per_member = ("out_of_sync", "max_lag", "sum_lag")
        out = {name: int(getattr(c, name)) for name, t in capi.ReplCensus._fields_ if name not in per_member}
        for name in per_member:
            out[name] = [int(x) for x in getattr(c, name)[:self.R]]
        return out

    def _hosting_request(self, close=None, open=None, self_slots=None):  # noqa: A002 (the header's name)
        """jg_node_hosting_request from the arguments of `close_groups` and `open_groups`; with it what it points at"""
        if self_slots is not None and open is None:
            raise EngineError(capi.EINVAL, "hosting: self_slots is for opening")
        hr, keep = capi.NodeHostingRequest(), []
        for field, groups, own in (("close", close, None), ("open", open, self_slots)):
            if groups is None:
                continue
            gs = self._group_set(groups, own, False, keep)
            keep.append(gs)
            setattr(hr, field, C.addressof(gs))
        return hr, keep

    def node_hosting(self) -> dict:
        """jg_node_hosting_view: the verdict of the hosting request that travelled with the kept step whose outbox
        `node_outbox` viewed last: {"redone": the step had general-path rows and the passes ran behind its catch-up pass
        (informational), "closed" / "opened": the slots each set wrote (its length, or 0), "close_refused" / "open_refused":
        the set met a slot in the wrong state and wrote nothing}.  A step that carried no request: {"redone": False}."""
        if not hasattr(self.api, "node_hosting_view"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}node_hosting_view")
        v = capi.NodeHosting()
        self._check(self.api.node_hosting_view(self._h, C.byref(v)))
        if not v.attached:
            return {"redone": False}
        return {"redone": bool(v.state & capi.NODE_POLL_REDONE), "closed": int(v.closed), "opened": int(v.opened),
                "close_refused": bool(v.state & capi.NODE_HOSTING_CLOSE_REFUSED), "open_refused": bool(v.state & capi.NODE_HOSTING_OPEN_REFUSED)}

    def _lookup_set(self, groups=None, g0: int = 0, n: Optional[int] = None, progress: bool = False):
        """jg_group_set of a lookup from the arguments of `lookup`; with it the list it points at"""
        s = capi.GroupSet()
        if groups is None:
            s.g0, s.n = int(g0), self.G - int(g0) if n is None else int(n)
            lst = None
        else:
            g = np.asarray(groups if isinstance(groups, np.ndarray) else list(groups)).reshape(-1)
            if g.size and (g.dtype.kind not in "iu" or int(g.min()) < 0 or int(g.max()) >= (1 << 32)):
                raise EngineError(capi.EINVAL, "slot index out of range")
            lst = np.ascontiguousarray(g, dtype=np.uint32)
            s.n, s.groups = lst.size, lst.ctypes.data if lst.size else None
        s.flags = capi.LOOKUP_PROGRESS if progress else 0
        return s, lst

    def node_lookup(self) -> dict:
        """jg_node_lookup_view: the answer of the point query that travelled with the kept step whose outbox `node_outbox`
        viewed last, as host copies: {"rows": what `lookup` returns for the same arguments (capi.GROUP_STATE_DTYPE),
        "match": [n, R] with progress=True, "redone": the step had general-path rows and the pass ran behind its catch-up
        pass (informational)}.  A step that carried no lookup: {"redone": False}."""
        if not hasattr(self.api, "node_lookup_view"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}node_lookup_view")
        v = capi.NodeLookup()
        self._check(self.api.node_lookup_view(self._h, C.byref(v)))
        if not v.attached:
            return {"redone": False}
        k = int(v.n)

        def arr(p, dtype, shape):
            if not k:
                return np.zeros(shape, dtype)
            nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return np.frombuffer((C.c_char * nbytes).from_address(p), dtype=dtype).reshape(shape).copy()

        out = {"rows": arr(v.rows, capi.GROUP_STATE_DTYPE, (k,)), "redone": bool(v.state & capi.NODE_POLL_REDONE)}
        if v.match:
            out["match"] = arr(v.match, np.uint64, (k, self.R))
        return out

    def lookup(self, groups=None, g0: int = 0, n: Optional[int] = None, progress: bool = False):
        """jg_engine_lookup_groups: the state of the listed slots, one row (capi.GROUP_STATE_DTYPE) per entry in the order
        asked - every read(...) field of the slot plus its leadership view (`state`, `known_leader`).  `groups`: any integer
        sequence or array, unsorted and with repeats; None: the range g0 .. g0 + n - 1.  With `progress`: (rows, match) with
        match[i, r] the progress head of replica r of entry i (0 for a slot that is not a leader)."""
        if not hasattr(self.api, "engine_lookup_groups"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_lookup_groups")
        s = capi.GroupSet()
        if groups is None:
            s.g0, s.n = int(g0), self.G - int(g0) if n is None else int(n)
            lst = None
        else:
            g = np.asarray(groups if isinstance(groups, np.ndarray) else list(groups)).reshape(-1)
            if g.size and (g.dtype.kind not in "iu" or int(g.min()) < 0 or int(g.max()) >= (1 << 32)):
                raise EngineError(capi.EINVAL, "slot index out of range")
            lst = np.ascontiguousarray(g, dtype=np.uint32)
            s.n, s.groups = lst.size, lst.ctypes.data
        rows = np.zeros(s.n, capi.GROUP_STATE_DTYPE)
        match = np.zeros((s.n, self.R), np.uint64) if progress else None
        s.flags = capi.LOOKUP_PROGRESS if progress else 0
        self._check(self.api.engine_lookup_groups(self._h, C.byref(s), rows.ctypes.data if s.n else None,
                                                  match.ctypes.data if progress else None))
        return (rows, match) if progress else rows

    def watch_commits(self, g0: int = 0, n: Optional[int] = None, limit: Optional[int] = None, peek: bool = False,
                      commits_only: bool = False, backlog: bool = False):
        """jg_engine_watch_commits: the slots of g0 .. g0 + n - 1 whose (commit, head) - with `commits_only` whose commit -
        differs from what this feed last delivered, ascending: (rows, total) with rows a structured array
        (capi.COMMIT_ROW_DTYPE: commit_from / head_from as last delivered, commit / head now) of the first `limit` of them
        and total their number; with `backlog` (rows, total, backlog) with the fields of jg_commit_backlog as a dict - every
        differing slot of the range before this call's delivery.  The delivered slots become "seen"; `peek` delivers the
        same rows and advances nothing.  One feed per engine."""
        n = self.G - int(g0) if n is None else int(n)
        if not hasattr(self.api, "engine_watch_commits"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_watch_commits")
        cap = n if limit is None else max(0, min(int(limit), n))
        out = np.zeros(max(cap, 1), capi.COMMIT_ROW_DTYPE)
        total = C.c_size_t(0)
        b = capi.CommitBacklog()
        flags = (capi.WATCH_PEEK if peek else 0) | (capi.WATCH_COMMITS_ONLY if commits_only else 0)
        self._check(self.api.engine_watch_commits(self._h, flags, int(g0), n, out.ctypes.data, cap, C.byref(total),
                                                  C.byref(b) if backlog else None))
        rows = out[:min(cap, total.value)]
        if not backlog:
            return rows, int(total.value)
        return rows, int(total.value), {name: int(getattr(b, name)) for name, _ in capi.CommitBacklog._fields_}

    def _await_api(self, name: str):
        if not hasattr(self.api, name):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}{name}")
        return getattr(self.api, name)

    def open_waiters(self, capacity: int) -> None:
        """jg_engine_await_open: (re)size the completion feed's table to `capacity` waiters (per shard on a multi-device
        handle); 0 frees it.  Refused while waiters are outstanding."""
        self._check(self._await_api("engine_await_open")(self._h, int(capacity)))

    def await_blocks(self, groups, block_ids, tokens, terms=0, deadlines_ms=0) -> int:
        """jg_engine_await_blocks: register one waiter per entry - (group, block id, token), guarded by `terms` where
        nonzero, expiring at `deadlines_ms` where nonzero; scalars broadcast.  All or nothing.  Returns the number
        registered."""
        fn = self._await_api("engine_await_blocks")
        groups = np.atleast_1d(np.asarray(groups))
        rows = np.zeros(len(groups), capi.AWAIT_ROW_DTYPE)
        if len(groups) and (groups.min() < 0 or groups.max() > 0xFFFFFFFF):
            raise EngineError(capi.EINVAL, "await_blocks: group out of range")
        rows["group"] = groups
        for name, v in (("block_id", block_ids), ("token", tokens), ("term", terms), ("deadline_ms", deadlines_ms)):
            rows[name] = np.asarray(v, dtype=np.uint64)
        self._check(fn(self._h, rows.ctypes.data, len(rows)))
        self._await_n = getattr(self, "_await_n", 0) + len(rows)
        return len(rows)

    def cancel_waiters(self, keys, mask: int = 2**64 - 1) -> int:
        """jg_engine_await_cancel (ABI v24): withdraw every outstanding waiter whose `token & mask` is among `keys` (any
        order, repeats allowed; at most capi.AWAIT_CANCEL_MAX) - exact tokens with the default mask, connections with
        mask=0xFFFFFFFF00000000 and `conn << 32` as keys, everything with keys=[0], mask=0.  The waiters are marked, not
        removed: the next `watch_completions` delivers them with state capi.DONE_CANCELLED, in registration order.  Returns
        the number newly marked."""
        fn = self._await_api("engine_await_cancel")
        keys = np.ascontiguousarray(np.atleast_1d(np.asarray(keys, dtype=np.uint64)))
        marked = C.c_size_t(0)
        self._check(fn(self._h, keys.ctypes.data if len(keys) else None, len(keys), int(mask), C.byref(marked)))
        return int(marked.value)

    def watch_completions(self, now_ms: int = 0, limit: Optional[int] = None, peek: bool = False, stats: bool = False):
        """jg_engine_watch_completions: the waiters that are done at `now_ms` - applied, lost or expired, the verdict in
        `state` (capi.DONE_*) - in registration order: (rows, total) with rows a structured array (capi.DONE_ROW_DTYPE) of
        the first `limit` of them and total their number; with `stats` (rows, total, stats) with the fields of
        jg_await_stats as a dict.  The delivered waiters leave the table; `peek` delivers the same rows and removes
        nothing."""
        fn = self._await_api("engine_watch_completions")
        have = getattr(self, "_await_n", 0)
        cap = have if limit is None else max(0, min(int(limit), have))
        out = np.zeros(max(cap, 1), capi.DONE_ROW_DTYPE)
        total = C.c_size_t(0)
        s = capi.AwaitStats()
        self._check(fn(self._h, capi.WATCH_PEEK if peek else 0, int(now_ms), out.ctypes.data, cap, C.byref(total),
                       C.byref(s) if stats else None))
        rows = out[:min(cap, total.value)]
        if not peek:
            self._await_n = have - len(rows)
        if not stats:
            return rows, int(total.value)
        return rows, int(total.value), {name: int(getattr(s, name)) for name, _ in capi.AwaitStats._fields_}

    def _poll_request(self, leaders=None, replicas=None, commits=None, census: bool = False, repl_census: Optional[int] = None,
                      g0: int = 0, n: Optional[int] = None):
        """the jg_poll of `poll`'s arguments: (p, what it points at - to be kept alive over the call, {"backlog": asked for})"""
        n = self.G - int(g0) if n is None else int(n)

        def options(arg, names, defaults):
            if arg is True:
                arg = {}
            if not isinstance(arg, dict):
                arg = dict(zip(names, tuple(arg)))
            unknown = set(arg) - set(names)
            if unknown:
                raise TypeError(f"poll: unknown option {sorted(unknown)}")
            return {**defaults, **arg}

        def rows_of(limit, dtype):
            cap = n if limit is None else max(0, min(int(limit), n))
            return cap, np.zeros(max(cap, 1), dtype)

        p = capi.Poll()
        p.g0, p.n = int(g0), n
        keep = {}
        if leaders is not None:
            o = options(leaders, ("limit", "peek"), dict(limit=None, peek=False))
            p.want |= capi.POLL_LEADERS
            p.leader_flags = capi.WATCH_PEEK if o["peek"] else 0
            p.leaders_cap, keep["leaders"] = rows_of(o["limit"], capi.LEADER_ROW_DTYPE)
            p.leaders = keep["leaders"].ctypes.data
        if replicas is not None:
            if isinstance(replicas, dict) and "now_ms" in replicas:  # the time rule
                if "leave_lag" in replicas:
                    raise TypeError("poll: replicas names now_ms (the time rule) and leave_lag (the lag rule)")
                o = options(replicas, ("now_ms", "max_behind_ms", "caught_lag", "join_lag", "limit", "peek"),
                            dict(caught_lag=0, join_lag=0, limit=None, peek=False))
                keep["clock"] = capi.IsrClock(int(o["now_ms"]), int(o["max_behind_ms"]), int(o["caught_lag"]), int(o["join_lag"]))
                p.clock = C.pointer(keep["clock"])
            else:
                o = options(replicas, ("leave_lag", "join_lag", "limit", "peek"), dict(join_lag=None, limit=None, peek=False))
                p.policy = capi.IsrPolicy(int(o["leave_lag"]), int(o["leave_lag"] if o["join_lag"] is None else o["join_lag"]))
            p.want |= capi.POLL_REPLICAS
            p.replica_flags = capi.WATCH_PEEK if o["peek"] else 0
            p.replicas_cap, keep["replicas"] = rows_of(o["limit"], capi.ISR_ROW_DTYPE)
            p.replicas = keep["replicas"].ctypes.data
        backlog = False
        if commits is not None:
            o = options(commits, ("limit", "peek", "commits_only", "backlog"), dict(limit=None, peek=False, commits_only=False, backlog=False))
            p.want |= capi.POLL_COMMITS
            p.commit_flags = (capi.WATCH_PEEK if o["peek"] else 0) | (capi.WATCH_COMMITS_ONLY if o["commits_only"] else 0)
            p.commits_cap, keep["commits"] = rows_of(o["limit"], capi.COMMIT_ROW_DTYPE)
            p.commits = keep["commits"].ctypes.data
            backlog = bool(o["backlog"])
        b, c, rc = capi.CommitBacklog(), capi.Census(), capi.ReplCensus()
        keep.update(backlog=b, census=c, repl_census=rc)
        if backlog:
            p.backlog = C.pointer(b)
        if census:
            p.want |= capi.POLL_CENSUS
            p.census = C.pointer(c)
        if repl_census is not None:
            p.want |= capi.POLL_REPL_CENSUS
            p.census_lag_limit = int(repl_census)
            p.repl_census = C.pointer(rc)
        return p, keep, {"backlog": backlog}

    def poll(self, leaders=None, replicas=None, commits=None, census: bool = False, repl_census: Optional[int] = None,
             g0: int = 0, n: Optional[int] = None) -> dict:
        """jg_engine_poll: the parts asked for of one tick over the slots g0 .. g0 + n - 1 in ONE call - one settle, one
        device pass, one synchronisation - each exactly as its separate method answers it.  A feed argument is None (not
        asked: its shadow is not touched), True, or that feed's options as a dict or a tuple in this order:
        leaders (limit, peek); replicas (leave_lag, join_lag, limit, peek); commits (limit, peek, commits_only, backlog).
        A `replicas` dict that names `now_ms` asks for the TIME rule (watch_replicas_timed; ABI v20): its keys are now_ms,
        max_behind_ms, caught_lag = 0, join_lag = 0, limit, peek - unless `peek`, the clocks of every slot of the range
        advance to now_ms, whatever `limit` is; naming leave_lag beside them is a TypeError.
        `census`: jg_engine_census too; `repl_census`: the lag limit of jg_engine_replication_census, or None.  Returns a
        dict keyed by the parts asked for: "leaders" / "replicas" (rows, total), "commits" (rows, total) or with backlog
        (rows, total, backlog), "census" / "repl_census" the dicts of census() / replication_census()."""
        if not hasattr(self.api, "engine_poll"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_poll")
        p, keep, parts = self._poll_request(leaders, replicas, commits, census, repl_census, g0, n)
        backlog, b, c, rc = parts["backlog"], keep["backlog"], keep["census"], keep["repl_census"]
        self._check(self.api.engine_poll(self._h, C.byref(p)))
        out = {}
        if leaders is not None:
            out["leaders"] = keep["leaders"][:min(p.leaders_cap, p.leaders_total)], int(p.leaders_total)
        if replicas is not None:
            out["replicas"] = keep["replicas"][:min(p.replicas_cap, p.replicas_total)], int(p.replicas_total)
        if commits is not None:
            out["commits"] = keep["commits"][:min(p.commits_cap, p.commits_total)], int(p.commits_total)
            if backlog:
                out["commits"] += ({name: int(getattr(b, name)) for name, _ in capi.CommitBacklog._fields_},)
        if census:
            out["census"] = self._census_dict(c)
        if repl_census is not None:
            out["repl_census"] = self._repl_census_dict(rc)
        return out

    def _census_dict(self, c) -> dict:
        out = {name: int(getattr(c, name)) for name, t in capi.Census._fields_ if name != "led_by"}
        out["led_by"] = [int(x) for x in c.led_by[:self.R]]
        return out

    def _repl_census_dict(self, rc) -> dict:
        per_member = ("out_of_sync", "max_lag", "sum_lag")
        out = {name: int(getattr(rc, name)) for name, t in capi.ReplCensus._fields_ if name not in per_member}
        for name in per_member:
            out[name] = [int(x) for x in getattr(rc, name)[:self.R]]
        return out

    def counters(self) -> dict:
        arr = (C.c_uint64 * 4)()
        self._check(self.api.get_counters(self._h, C.byref(arr)))
        return {"commands": arr[0], "decisions": arr[1], "dense_group_steps": arr[2], "launches": arr[3]}

    def snapshot(self) -> dict:
        """All readable columns (used by the parity tests)."""
        snap = {}
        for name in capi.FIELD_NAMES:
            if name == "match":
                snap[name] = np.stack([self.read("match", r) for r in range(self.R)])
            else:
                snap[name] = self.read(name)
        return snap

    def chain_compact(self, trees: Iterable[Tuple[Sequence[Tuple[int, int]], int]]) -> List[np.ndarray]:
        """Batched Chain::compact: trees = [([(id, next), ...], commit), ...] -> removed masks."""
        trees = list(trees)
        off = np.zeros(len(trees) + 1, np.uint64)
        for i, (blocks, _) in enumerate(trees):
            off[i + 1] = off[i] + len(blocks)
        ids = np.array([b[0] for t in trees for b in t[0]], dtype=np.uint64)
        nexts = np.array([b[1] for t in trees for b in t[0]], dtype=np.uint64)
        commits = np.array([t[1] for t in trees], dtype=np.uint64)
        removed = np.zeros(int(off[-1]), np.uint8)
        ids = np.ascontiguousarray(ids)
        nexts = np.ascontiguousarray(nexts)
        self._check(self.api.chain_compact(self._h, len(trees), off.ctypes.data, ids.ctypes.data,
                                           nexts.ctypes.data, commits.ctypes.data, removed.ctypes.data))
        return [removed[int(off[i]):int(off[i + 1])].copy() for i in range(len(trees))]

    def load_chains(self, trees=None, now_ms: int = 0, g0: int = 0, *, off=None, blk_id=None, blk_next=None,
                    commit=None, has_commit=None) -> None:
        """jg_engine_load_chains: groups g0, g0 + 1, ... restart on the persisted trees given - Raft::<Follower>::new +
        Chain::new on each (follower.rs:68-95, chain.rs:117-137).  Either `trees` = [(blocks [(id, next), ...] in
        ascending id order, commit key value or None), ...] one per group, or the CSR arrays directly (off [n + 1],
        blk_id / blk_next [off[n]], commit [n], has_commit [n])."""
        self._flush_pending()
        if trees is not None:
            trees = list(trees)
            n = len(trees)
            off = np.zeros(n + 1, np.uint64)
            off[1:] = np.cumsum([len(t[0]) for t in trees], dtype=np.uint64) if n else []
            rows = [b for t in trees for b in t[0]]
            blk_id = np.array([b[0] for b in rows], dtype=np.uint64)
            blk_next = np.array([b[1] for b in rows], dtype=np.uint64)
            commit = np.array([0 if t[1] is None else t[1] for t in trees], dtype=np.uint64)
            has_commit = np.array([t[1] is not None for t in trees], dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        blk_id = np.ascontiguousarray(blk_id if blk_id is not None else [], dtype=np.uint64)
        blk_next = np.ascontiguousarray(blk_next if blk_next is not None else [], dtype=np.uint64)
        commit = np.ascontiguousarray(commit if commit is not None else np.zeros(n), dtype=np.uint64)
        has_commit = np.ascontiguousarray(has_commit if has_commit is not None else np.zeros(n), dtype=np.uint8)
        assert n >= 0 and len(commit) == n and len(has_commit) == n and len(blk_id) == len(blk_next)
        img = capi.ChainImage()
        img.g0, img.n = int(g0), n
        img.off, img.blk_id, img.blk_next = off.ctypes.data, blk_id.ctypes.data, blk_next.ctypes.data
        img.commit, img.has_commit = commit.ctypes.data, has_commit.ctypes.data
        if not hasattr(self.api, "engine_load_chains"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_load_chains")
        self._check(self.api.engine_load_chains(self._h, int(now_ms), C.byref(img)))

    def read_chains(self, g0: int = 0, n: Optional[int] = None, from_=None) -> dict:
        """jg_engine_read_chains: groups g0 .. g0 + n - 1 as a sled scan of each tree (the inverse of load_chains):
        dict of off [n + 1], blk_id / blk_next [off[n]] (ids ascending within a group), commit [n], has_commit [n] and
        fault [n].  `from_` [n]: only the block keys >= from_[i] (Chain::range(from..)).  Sized first, then read."""
        n = self.G - g0 if n is None else int(n)
        if not hasattr(self.api, "engine_read_chains"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_read_chains")
        fr = None if from_ is None else np.ascontiguousarray(from_, dtype=np.uint64)
        assert fr is None or len(fr) == n
        out = dict(off=np.zeros(n + 1, np.uint64), commit=np.zeros(n, np.uint64), has_commit=np.zeros(n, np.uint8),
                   fault=np.zeros(n, np.uint8))
        r = capi.ChainRead()
        r.g0, r.n = int(g0), n
        r.from_ = 0 if fr is None else fr.ctypes.data
        r.off, r.commit = out["off"].ctypes.data, out["commit"].ctypes.data
        r.has_commit, r.fault = out["has_commit"].ctypes.data, out["fault"].ctypes.data
        rows = C.c_uint64(0)
        rc = self.api.engine_read_chains(self._h, C.byref(r), C.byref(rows))  # the sizing call (cap 0)
        if rc == capi.ECAPACITY:
            out["blk_id"] = np.zeros(rows.value, np.uint64)
            out["blk_next"] = np.zeros(rows.value, np.uint64)
            r.cap, r.blk_id, r.blk_next = rows.value, out["blk_id"].ctypes.data, out["blk_next"].ctypes.data
            rc = self.api.engine_read_chains(self._h, C.byref(r), C.byref(rows))
        else:
            out["blk_id"], out["blk_next"] = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        self._check(rc)
        return out

    def read_trees(self, g0: int = 0, n: Optional[int] = None, from_=None) -> list:
        """read_chains in the form load_chains(trees=...) takes: [(blocks [(id, next), ...], commit key value or None),
        ...] one per group; None for a group whose sticky fault is engine-domain (>= 128: its image is not its tree)."""
        r = self.read_chains(g0, n, from_)
        off, ids, nxt = r["off"].astype(np.int64), r["blk_id"].tolist(), r["blk_next"].tolist()
        out = []
        for i in range(len(r["commit"])):
            if r["fault"][i] >= 128:
                out.append(None)
                continue
            blocks = list(zip(ids[off[i]:off[i + 1]], nxt[off[i]:off[i + 1]]))
            out.append((blocks, int(r["commit"][i]) if r["has_commit"][i] else None))
        return out

    def export_groups(self, g0: int = 0, n: Optional[int] = None, device: bool = False) -> "GroupImage":
        """jg_engine_export_groups: the full state of groups g0 .. g0 + n - 1 as a GroupImage (header fields plus one
        record per group: numpy uint8 [n, record_bytes], or with `device` a buffer in this engine's device memory).
        Changes nothing; import_groups on another engine of the same node continues the groups bit for bit."""
        n = self.G - g0 if n is None else int(n)
        if not hasattr(self.api, "engine_export_groups"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_export_groups")
        x = capi.GroupExport()
        x.g0, x.n, x.flags = int(g0), n, capi.MOVE_DEVICE if device else 0
        rc = self.api.engine_export_groups(self._h, C.byref(x))  # the sizing call (cap 0): the header
        if rc != capi.ECAPACITY:
            self._check(rc)
        nbytes = n * x.header.record_bytes
        if device:
            p = C.c_void_p()
            self._check(self.api.device_alloc(self._h, max(nbytes, 16), C.byref(p)))
            img = GroupImage(x.header, g0=int(g0), device_ptr=p, owner=self)
            x.records = p.value
        else:
            img = GroupImage(x.header, g0=int(g0), records=np.zeros((n, x.header.record_bytes), np.uint8))
            x.records = img.records.ctypes.data
        x.cap_bytes = nbytes
        self._check(self.api.engine_export_groups(self._h, C.byref(x)))
        return img

    def import_groups(self, image: "GroupImage", g0: Optional[int] = None, shift_ms: int = 0) -> None:
        """jg_engine_import_groups: the image's groups continue at local groups g0 .. g0 + n - 1 (default: the indices
        they were exported from); `shift_ms` is added (wrapping) to their election and heartbeat times."""
        if not hasattr(self.api, "engine_import_groups"):
            raise EngineError(capi.EINVAL, f"{self.api.path} does not export {self.api.prefix}engine_import_groups")
        self._flush_pending()
        x = capi.GroupImport()
        x.g0 = image.g0 if g0 is None else int(g0)
        x.shift_ms = int(shift_ms)
        x.header = image.header
        if image.device_ptr is not None:
            x.flags, x.records = capi.MOVE_DEVICE, image.device_ptr.value
        else:
            rec = np.ascontiguousarray(image.records, dtype=np.uint8)
            x.records = rec.ctypes.data
        self._check(self.api.engine_import_groups(self._h, C.byref(x)))

    def chain_compact_resident(self) -> np.ndarray:
        """jg_chain_compact_resident + jg_drain_compacted: Chain::compact on every healthy group's own
        chain; returns the removed blocks as (group, id) rows, group ascending, ids in walk order."""
        self._flush_pending()
        n = C.c_size_t(0)
        self._check(self.api.chain_compact_resident(self._h, C.byref(n)))
        return self._drain(self.api.drain_compacted, capi.COMPACT_DTYPE)

    def handle(self, group: int) -> "RaftHandle":
        return RaftHandle(self, group)


class GroupImage:
    """A state image of jg_engine_export_groups: the header's fields (format, record_bytes, n, n_replicas, node_ids,
    separate_commit_key, seed, global0), `g0` (the local index the records were exported from) and the records - a numpy
    uint8 [n, record_bytes] array, or `device_ptr` in the exporting engine's device memory (freed with the image)."""

    def __init__(self, header, g0: int = 0, records: Optional[np.ndarray] = None, device_ptr=None, owner=None):
        self.header = capi.GroupImageHeader()
        C.pointer(self.header)[0] = header
        self.g0, self.records, self.device_ptr, self._owner = int(g0), records, device_ptr, owner
        for f, *_ in capi.GroupImageHeader._fields_:
            if f != "reserved":
                v = getattr(self.header, f)
                setattr(self, f, list(v)[:self.header.n_replicas] if f == "node_ids" else int(v))

    def to_host(self) -> np.ndarray:
        """the records as numpy uint8 [n, record_bytes] (a download of the device form)"""
        if self.device_ptr is None:
            return self.records
        out = np.zeros((self.n, self.record_bytes), np.uint8)
        if out.nbytes:
            self._owner._check(self._owner.api.device_download(self._owner._h, out.ctypes.data, self.device_ptr, out.nbytes))
        return out

    def free(self) -> None:
        if self.device_ptr is not None and self._owner is not None and getattr(self._owner, "_h", None):
            self._owner.api.device_free(self._owner._h, self.device_ptr)
        self.device_ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def move_groups(src: BatchedRaft, dst: BatchedRaft, g0: int, n: int, dst_g0: Optional[int] = None, shift_ms: int = 0,
                close_source: bool = False) -> None:
    """Hand groups g0 .. g0 + n - 1 of `src` over to `dst` (at dst_g0, default g0) without a restart: export, import.
    The caller stops driving them on `src` afterwards - or, with `close_source`, the hosted ones among them are closed on
    `src` once the import has succeeded (vacant slots: src emits nothing more for them, under any step)."""
    img = src.export_groups(g0, n)
    dst.import_groups(img, g0 if dst_g0 is None else dst_g0, shift_ms)
    if close_source:
        hosted = src.hosted_groups(g0, n)
        if hosted.size:
            src.close_groups(hosted)


class Shard(_Hosting):
    """One shard of a multi-device BatchedRaft: a borrowed engine handle (owned by the parent)
    plus the group range it owns.  Quacks enough like a BatchedRaft for the device-pointer calls (open_groups /
    close_groups with `device`: shard-local indices in the shard's device memory)."""

    def __init__(self, parent: BatchedRaft, info: "capi.ShardInfo"):
        self.parent, self.api = parent, parent.api
        self._h = C.c_void_p(info.engine)
        self.device_id, self.group_lo, self.G, self.R = info.device_id, info.group_lo, info.n_groups, parent.R
        self.node_ids = parent.node_ids
        self._check = parent._check

    def alloc(self, nbytes: int) -> C.c_void_p:
        p = C.c_void_p()
        self._check(self.api.device_alloc(self._h, nbytes, C.byref(p)))
        return p

    def upload(self, dev_ptr, host: np.ndarray) -> None:
        host = np.ascontiguousarray(host)
        self._check(self.api.device_upload(self._h, dev_ptr, host.ctypes.data, host.nbytes))


class RaftHandle:
    """enum RaftHandle (src/raft/mod.rs:417-468) for one group of a BatchedRaft."""

    def __init__(self, engine: BatchedRaft, group: int):
        self.engine = engine
        self.group = int(group)

    def apply(self, cmd: Command, now_ms: int = 0) -> "RaftHandle":
        return self.engine.apply(self.group, cmd, now_ms)

    def _get(self, name: str, replica: int = 0):
        return self.engine.read(name, replica, self.group, 1)[0]

    def is_follower(self) -> bool:
        return self._get("role") == capi.ROLE_FOLLOWER

    def is_candidate(self) -> bool:
        return self._get("role") == capi.ROLE_CANDIDATE

    def is_leader(self) -> bool:
        return self._get("role") == capi.ROLE_LEADER

    @property
    def id(self) -> int:
        return self.engine.node_ids[int(self._get("self_slot"))]

    @property
    def current_term(self) -> int:
        return int(self._get("term"))

    @property
    def voted_for(self) -> Optional[int]:
        return int(self._get("voted_for")) if self._get("has_voted") else None

    @property
    def commit(self) -> int:
        return int(self._get("commit"))

    @property
    def head(self) -> int:
        return int(self._get("head"))

    @property
    def fault(self) -> int:
        return int(self._get("fault"))

    def match(self, replica: int) -> int:
        return int(self._get("match", replica))


class DeviceRows:
    """A command batch resident in device memory (see BatchedRaft.upload_rows)."""

    def __init__(self, engine: BatchedRaft, cols, side):
        self.engine = engine
        self.n = len(cols[0])
        self._ptrs = []
        api, h = engine.api, engine._h

        def up(a):
            p = C.c_void_p()
            engine._check(api.device_alloc(h, max(a.nbytes, 16), C.byref(p)))
            if a.nbytes:
                engine._check(api.device_upload(h, p, a.ctypes.data, a.nbytes))
            self._ptrs.append(p)
            return p.value

        b = capi.CmdBatch()
        b.n = self.n
        (b.kind, b.group, b.from_, b.term, b.id, b.aux, b.flag) = [up(c) for c in cols]
        b.n_blocks = len(side[0])
        b.blk_id, b.blk_next = up(side[0]), up(side[1])
        self.batch = b

    def free(self) -> None:
        for p in self._ptrs:
            self.engine.api.device_free(self.engine._h, p)
        self._ptrs = []


class DeviceList:
    """uint32 values in device memory (jg_device_alloc + jg_device_upload); .ptr is the device address."""

    def __init__(self, engine, values: np.ndarray):
        self.engine, self.n = engine, len(values)
        p = C.c_void_p()
        engine._check(engine.api.device_alloc(engine._h, max(values.nbytes, 16), C.byref(p)))
        self._p = p
        if values.nbytes:
            engine._check(engine.api.device_upload(engine._h, p, values.ctypes.data, values.nbytes))

    @property
    def ptr(self) -> int:
        return self._p.value

    def free(self) -> None:
        if self._p:
            self.engine.api.device_free(self.engine._h, self._p)
            self._p = None


class DenseCluster:
    """jg_dense_cluster: the R nodes of every partition as R engines of one process, their
    protocol rounds driven from inside the library (josefine_gpu.h, "a closed loop of dense node
    ticks").  `nodes[r]` hosts replica slot r of every group; nodes[lead] is made leader by the
    caller (traces.elect_all)."""

    def __init__(self, nodes, lead=0, vote_words=False):
        """lead = None: per-partition leadership (JG_CLUSTER_ANY_LEADER) - every node leads the partitions it was
        elected for and follows the others.  vote_words: JG_CLUSTER_OPT_VOTE_WORDS (an election's traffic of the routed
        round as mailbox words, csrc/jg_votes.h)."""
        self.nodes, self.lead, self.R = list(nodes), lead, len(nodes)
        self.api = nodes[0].api
        arr = (C.c_void_p * self.R)(*[n._h for n in nodes])
        self._h = C.c_void_p()
        nodes[0]._check(self.api.dense_cluster_create(arr, self.R, capi.CLUSTER_ANY_LEADER if lead is None else lead, C.byref(self._h)))
        self.vote_words = bool(vote_words)
        if vote_words:
            self.set_option(capi.CLUSTER_OPT_VOTE_WORDS, 1)

    def set_option(self, option: int, value: int) -> None:
        self.nodes[0]._check(self.api.dense_cluster_set_option(self._h, int(option), int(value)))

    def close(self) -> None:
        if self._h:
            self.api.dense_cluster_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # (this object keeps its nodes alive: the cluster always goes before them)
        try:
            self.close()
        except Exception:
            pass

    def set_appends(self, uniform: int = 1, per_group=None) -> None:
        p = None if per_group is None else np.ascontiguousarray(per_group, dtype=np.uint64).ctypes.data
        self.nodes[0]._check(self.api.dense_cluster_set_appends(self._h, int(uniform), p))

    def withdraw_appends(self, groups_dev_ptr: int, n: int) -> None:
        """jg_dense_cluster_withdraw_appends: no more ClientRequests for the n groups listed in device memory."""
        self.nodes[0]._check(self.api.dense_cluster_withdraw_appends(self._h, C.c_void_p(groups_dev_ptr), int(n)))

    def offer_appends(self, groups_dev_ptr: int, n: int, per_round: int) -> None:
        """jg_dense_cluster_offer_appends: `per_round` ClientRequests per round for the n groups listed in device memory."""
        self.nodes[0]._check(self.api.dense_cluster_offer_appends(self._h, C.c_void_p(groups_dev_ptr), int(n), int(per_round)))

    def rounds(self, now_ms: int, dt_ms: int, n: int) -> None:
        self.nodes[0]._check(self.api.dense_cluster_rounds(self._h, int(now_ms), int(dt_ms), int(n)))

    def round_routed(self, now_ms: int, inject=None) -> dict:
        """jg_dense_cluster_round_routed; `inject`: per node a DeviceRows (upload_rows) or None."""
        arr = None
        if inject is not None:
            arr = (capi.CmdBatch * self.R)()
            for r, rows in enumerate(inject):
                if rows is not None:
                    arr[r] = rows.batch
        st = capi.RouteStats()
        self.nodes[0]._check(self.api.dense_cluster_round_routed(self._h, int(now_ms), arr, C.byref(st)))
        return {"delivered": [int(st.delivered[r]) for r in range(self.R)], "kept": int(st.kept), "fsm_rows": int(st.fsm_rows)}
