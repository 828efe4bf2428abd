"""ctypes view of include/josefine_gpu.h.

The same table binds any shared library that exports the ABI under a symbol
prefix: the shipped HIP engine uses ``jg_``; the test-suite binds its CPU
checker (prefix ``jo_``) through the very same table so both are driven by
identical code.  Nothing in this package loads that checker.
"""
from __future__ import annotations

import ctypes as C

ABI_VERSION = 26
CLUSTER_ANY_LEADER = 0xFFFFFFFF
CLUSTER_OPT_VOTE_WORDS = 1
MAX_REPLICAS = 8
CHAIN_WINDOW = 8
MAX_INFLIGHT = 5
MAX_DEVICES = 16
FOREIGN_VOTERS = 8
MAX_DENSE_APPENDS = 1 << 20
NO_ACK = 0xFFFFFFFFFFFFFFFF
AEC_INDIVIDUAL = 0xFFFFFFFFFFFFFFFE  # jg_node_outbox.aec: the partition's AppendEntries words differ by addressee (see .ae)

OK, EINVAL, ENOMEM, EDEVICE, ECAPACITY = 0, -1, -2, -3, -4

ROLE_FOLLOWER, ROLE_CANDIDATE, ROLE_LEADER = 0, 1, 2

(CMD_TICK, CMD_PROPOSE, CMD_VOTE_REQUEST, CMD_VOTE_RESPONSE, CMD_APPEND_ENTRIES,
 CMD_APPEND_RESPONSE, CMD_HEARTBEAT, CMD_HEARTBEAT_RESPONSE, CMD_TIMEOUT, CMD_NOOP,
 CMD_CLIENT_REQUEST, CMD_CLIENT_RESPONSE, CMD_RESTART, CMD_RECREATE) = range(14)

TO_PEERS, TO_PEER, TO_LOCAL, TO_CLIENT, TO_QUEUE = range(5)
QUEUE_FLUSH, QUEUE_DROP = 1, 2

FAULT_NONE = 0
FAULT_LEADER_TERM_UNIMPLEMENTED = 1
FAULT_APPEND_ID_NOT_ABOVE_HEAD = 2
FAULT_PROGRESS_UNKNOWN_NODE = 3
FAULT_COMMIT_MISSING_BLOCK = 4
FAULT_EXTEND_MISSING_PARENT = 5
FAULT_FOLLOWER_STALE_LEADER = 6
FAULT_CANDIDATE_TICK_ELECTED = 7
FAULT_RANGE_HIT_COMMIT_KEY = 8
FAULT_ENGINE_WINDOW_OVERFLOW = 128
FAULT_ENGINE_FOREIGN_VOTER = 129
FAULT_ENGINE_DENSE_NONLEADER = 131
FAULT_ENGINE_DENSE_APPENDS = 132
FAULT_ENGINE_MAILBOX_RANGE = 133
FAULT_VACANT = 255  # not a fault: the slot hosts no partition

CFG_SEPARATE_COMMIT_KEY = 1
CFG_FLAT_ROW_PASSES = 2  # jg_step_node's row passes untiled (the tiled ones' statement; an A/B)
CFG_START_VACANT = 4  # every slot starts vacant
NODE_LEADER_HALF, NODE_FOLLOWER_HALF, NODE_TICK, NODE_ASYNC, NODE_COMMON_AE, NODE_FSM_FUSED, NODE_KEEP = 1, 2, 4, 8, 16, 32, 64

FSM_APPLY_LEADER, FSM_APPLY_FOLLOWER, FSM_NOTIFY, FSM_LEADER_STEP = 0, 1, 2, 3

(FIELD_TERM, FIELD_VOTED_FOR, FIELD_HAS_VOTED, FIELD_ROLE, FIELD_COMMIT, FIELD_HEAD,
 FIELD_ID_GEN, FIELD_MATCH, FIELD_REPL_STATE, FIELD_VOTE_SEEN, FIELD_VOTE_GRANTED,
 FIELD_FAULT, FIELD_LEADER_ID, FIELD_HAS_LEADER, FIELD_ELECTION_TIME,
 FIELD_ELECTION_TIMEOUT, FIELD_HEARTBEAT_TIME, FIELD_QUEUED_REQS, FIELD_SELF_SLOT) = range(19)

# numpy dtype per readable column
FIELD_DTYPES = {
    FIELD_TERM: "u8", FIELD_VOTED_FOR: "u4", FIELD_HAS_VOTED: "u1", FIELD_ROLE: "u1",
    FIELD_COMMIT: "u8", FIELD_HEAD: "u8", FIELD_ID_GEN: "u8", FIELD_MATCH: "u8",
    FIELD_REPL_STATE: "u1", FIELD_VOTE_SEEN: "u1", FIELD_VOTE_GRANTED: "u1", FIELD_FAULT: "u1",
    FIELD_LEADER_ID: "u4", FIELD_HAS_LEADER: "u1", FIELD_ELECTION_TIME: "u8",
    FIELD_ELECTION_TIMEOUT: "u4", FIELD_HEARTBEAT_TIME: "u8", FIELD_QUEUED_REQS: "u4",
    FIELD_SELF_SLOT: "u1",
}
FIELD_NAMES = {
    "term": FIELD_TERM, "voted_for": FIELD_VOTED_FOR, "has_voted": FIELD_HAS_VOTED,
    "role": FIELD_ROLE, "commit": FIELD_COMMIT, "head": FIELD_HEAD, "id_gen": FIELD_ID_GEN,
    "match": FIELD_MATCH, "repl_state": FIELD_REPL_STATE, "vote_seen": FIELD_VOTE_SEEN,
    "vote_granted": FIELD_VOTE_GRANTED, "fault": FIELD_FAULT, "leader_id": FIELD_LEADER_ID,
    "has_leader": FIELD_HAS_LEADER, "election_time": FIELD_ELECTION_TIME,
    "election_timeout": FIELD_ELECTION_TIMEOUT, "heartbeat_time": FIELD_HEARTBEAT_TIME,
    "queued_reqs": FIELD_QUEUED_REQS, "self_slot": FIELD_SELF_SLOT,
}


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32),
        ("n_groups", C.c_uint32),
        ("n_replicas", C.c_uint32),
        ("node_ids", C.c_uint32 * MAX_REPLICAS),
        ("device_id", C.c_int32),
        ("heartbeat_timeout_ms", C.c_uint32),
        ("election_timeout_min_ms", C.c_uint32),
        ("election_timeout_max_ms", C.c_uint32),
        ("seed", C.c_uint64),
        ("group_base", C.c_uint64),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("n_devices", C.c_uint32),
        ("device_ids", C.c_int32 * MAX_DEVICES),
    ]


class ShardInfo(C.Structure):
    _fields_ = [("engine", C.c_void_p), ("device_id", C.c_int32), ("group_lo", C.c_uint32),
                ("n_groups", C.c_uint32), ("reserved", C.c_uint32)]


class RouteStats(C.Structure):
    """jg_route_stats."""
    _fields_ = [("delivered", C.c_uint64 * 8), ("kept", C.c_uint64), ("fsm_rows", C.c_uint64)]


class NodeOutbox(C.Structure):
    """jg_node_outbox."""
    _fields_ = [("beat", C.c_void_p), ("ae", C.c_void_p), ("answer", C.c_void_p), ("hb_commit", C.c_void_p),
                ("rows", C.c_uint64), ("rows_general", C.c_uint64), ("bytes_h2d", C.c_uint64), ("bytes_d2h", C.c_uint64),
                ("aec", C.c_void_p)]


class CmdCols(C.Structure):
    """jg_cmd_cols."""
    _fields_ = [(k, C.c_void_p) for k in ("kind", "group", "from_", "term", "id", "aux", "flag", "blk_id", "blk_next")]


COL_FROM, COL_TERM, COL_AUX, COL_FLAG, COL_UNCHECKED, COL_UPLOAD_NOW, COL_PACKED_KIND, COL_ID32 = 1, 2, 4, 8, 16, 32, 64, 128


class CmdBatch(C.Structure):
    _fields_ = [
        ("n", C.c_size_t),
        ("kind", C.c_void_p),
        ("group", C.c_void_p),
        ("from_", C.c_void_p),
        ("term", C.c_void_p),
        ("id", C.c_void_p),
        ("aux", C.c_void_p),
        ("flag", C.c_void_p),
        ("n_blocks", C.c_size_t),
        ("blk_id", C.c_void_p),
        ("blk_next", C.c_void_p),
    ]


AE_NONE = 0xFF
HB_NONE = 0xFF


class LeaderInbox(C.Structure):
    _fields_ = [("answers", C.c_void_p), ("hbr_commit", C.c_void_p)]


class LeaderOutbox(C.Structure):
    _fields_ = [("beat", C.c_void_p), ("ae", C.c_void_p)]


class FollowerInbox(C.Structure):
    _fields_ = [("leader", C.c_void_p), ("leader_id", C.c_uint32), ("reserved", C.c_uint32),
                ("beat", C.c_void_p), ("ae", C.c_void_p)]


class FollowerOutbox(C.Structure):
    _fields_ = [("answer", C.c_void_p), ("hb_commit", C.c_void_p)]


class ChainImage(C.Structure):
    _fields_ = [("g0", C.c_uint32), ("n", C.c_uint32), ("off", C.c_void_p), ("blk_id", C.c_void_p),
                ("blk_next", C.c_void_p), ("commit", C.c_void_p), ("has_commit", C.c_void_p)]


class ChainRead(C.Structure):
    _fields_ = [("g0", C.c_uint32), ("n", C.c_uint32), ("from_", C.c_void_p), ("cap", C.c_uint64), ("off", C.c_void_p),
                ("blk_id", C.c_void_p), ("blk_next", C.c_void_p), ("commit", C.c_void_p), ("has_commit", C.c_void_p),
                ("fault", C.c_void_p)]


MOVE_FORMAT = 1
MOVE_DEVICE = 1


class GroupImageHeader(C.Structure):
    _fields_ = [("format", C.c_uint32), ("record_bytes", C.c_uint32), ("n", C.c_uint32), ("n_replicas", C.c_uint32),
                ("node_ids", C.c_uint32 * MAX_REPLICAS), ("separate_commit_key", C.c_uint32), ("reserved", C.c_uint32),
                ("seed", C.c_uint64), ("global0", C.c_uint64)]


class GroupExport(C.Structure):
    _fields_ = [("g0", C.c_uint32), ("n", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("cap_bytes", C.c_uint64), ("records", C.c_void_p), ("header", GroupImageHeader)]


class GroupImport(C.Structure):
    _fields_ = [("g0", C.c_uint32), ("flags", C.c_uint32), ("shift_ms", C.c_int64), ("records", C.c_void_p),
                ("header", GroupImageHeader)]


GROUPS_DEVICE = 1
LOOKUP_PROGRESS = 2  # jg_group_set.flags of jg_engine_lookup_groups
LIST_VACANT = 0
LIST_HOSTED = 1


class GroupSet(C.Structure):
    _fields_ = [("g0", C.c_uint32), ("n", C.c_uint32), ("groups", C.c_void_p), ("self_slots", C.c_void_p),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


LEAD_KNOWN, LEAD_SELF, LEAD_VACANT, LEAD_FAULTED = 1, 2, 4, 8  # jg_leader_row.state
WATCH_PEEK = 1
WATCH_COMMITS_ONLY = 2  # flags of jg_engine_watch_commits


class LeaderRow(C.Structure):
    """jg_leader_row."""
    _fields_ = [("group", C.c_uint32), ("leader_id", C.c_uint32), ("term", C.c_uint64), ("role", C.c_uint8), ("state", C.c_uint8),
                ("fault", C.c_uint8), ("self_slot", C.c_uint8), ("reserved", C.c_uint32)]


class Census(C.Structure):
    """jg_census."""
    _fields_ = [("hosted", C.c_uint64), ("vacant", C.c_uint64), ("faulted_reference", C.c_uint64), ("faulted_engine", C.c_uint64),
                ("followers", C.c_uint64), ("candidates", C.c_uint64), ("leaders", C.c_uint64), ("leaderless", C.c_uint64),
                ("led_by", C.c_uint64 * MAX_REPLICAS), ("led_by_other", C.c_uint64), ("max_term", C.c_uint64),
                ("uncommitted", C.c_uint64)]


ISR_LEADS, ISR_UNDER, ISR_BELOW_QUORUM = 1, 2, 4  # jg_isr_row.state


class IsrPolicy(C.Structure):
    """jg_isr_policy."""
    _fields_ = [("leave_lag", C.c_uint64), ("join_lag", C.c_uint64)]


class IsrClock(C.Structure):
    """jg_isr_clock."""
    _fields_ = [("now_ms", C.c_uint64), ("max_behind_ms", C.c_uint64), ("caught_lag", C.c_uint64), ("join_lag", C.c_uint64)]


# jg_commit_row.state
CMT_COMMITTED, CMT_APPENDED, CMT_REWOUND, CMT_LEADS, CMT_VACANT, CMT_FAULTED = 1, 2, 4, 8, 16, 32


class CommitBacklog(C.Structure):
    """jg_commit_backlog."""
    _fields_ = [("changed", C.c_uint64), ("committed", C.c_uint64), ("appended", C.c_uint64), ("rewound", C.c_uint64),
                ("pending_commits", C.c_uint64), ("pending_appends", C.c_uint64)]


class ReplCensus(C.Structure):
    """jg_repl_census."""
    _fields_ = [("leaders", C.c_uint64), ("fully_replicated", C.c_uint64), ("under_replicated", C.c_uint64),
                ("below_quorum", C.c_uint64), ("out_of_sync", C.c_uint64 * MAX_REPLICAS), ("max_lag", C.c_uint64 * MAX_REPLICAS),
                ("sum_lag", C.c_uint64 * MAX_REPLICAS), ("max_uncommitted", C.c_uint64)]


# jg_done_row.state
DONE_APPLIED, DONE_LOST, DONE_EXPIRED, DONE_VACANT, DONE_FAULTED, DONE_CANCELLED = 1, 2, 4, 8, 16, 32
AWAIT_WITHDRAWN = 1  # jg_await_row.flags as the table keeps it (never accepted from a caller)
AWAIT_CANCEL_MAX = 65536  # jg_engine_await_cancel: the most keys of one call


class AwaitStats(C.Structure):
    """jg_await_stats."""
    _fields_ = [("waiting", C.c_uint64), ("done", C.c_uint64), ("applied", C.c_uint64), ("lost", C.c_uint64),
                ("expired", C.c_uint64), ("left", C.c_uint64)]


POLL_LEADERS, POLL_REPLICAS, POLL_COMMITS, POLL_CENSUS, POLL_REPL_CENSUS = 1, 2, 4, 8, 16  # jg_poll.want


class Poll(C.Structure):
    """jg_poll."""
    _fields_ = [("want", C.c_uint32), ("g0", C.c_uint32), ("n", C.c_uint32), ("leader_flags", C.c_uint32),
                ("replica_flags", C.c_uint32), ("commit_flags", C.c_uint32), ("policy", IsrPolicy), ("census_lag_limit", C.c_uint64),
                ("leaders", C.c_void_p), ("leaders_cap", C.c_size_t), ("leaders_total", C.c_size_t),
                ("replicas", C.c_void_p), ("replicas_cap", C.c_size_t), ("replicas_total", C.c_size_t),
                ("commits", C.c_void_p), ("commits_cap", C.c_size_t), ("commits_total", C.c_size_t),
                ("backlog", C.POINTER(CommitBacklog)), ("census", C.POINTER(Census)), ("repl_census", C.POINTER(ReplCensus)),
                ("clock", C.POINTER(IsrClock))]


NODE_POLL_REDONE = 1  # jg_node_poll.state


class NodePoll(C.Structure):
    """jg_node_poll."""
    _fields_ = [("want", C.c_uint32), ("state", C.c_uint32),
                ("leaders", C.c_void_p), ("leaders_n", C.c_size_t), ("leaders_total", C.c_size_t),
                ("replicas", C.c_void_p), ("replicas_n", C.c_size_t), ("replicas_total", C.c_size_t),
                ("commits", C.c_void_p), ("commits_n", C.c_size_t), ("commits_total", C.c_size_t),
                ("backlog", CommitBacklog), ("census", Census), ("repl_census", ReplCensus)]


class NodeAwaitRequest(C.Structure):
    """jg_node_await_request."""
    _fields_ = [("rows", C.c_void_p), ("n", C.c_size_t), ("flags", C.c_uint32), ("want_stats", C.c_uint32), ("now_ms", C.c_uint64),
                ("cap", C.c_size_t), ("cancel_keys", C.c_void_p), ("cancel_n", C.c_size_t), ("cancel_mask", C.c_uint64)]


class NodeAwait(C.Structure):
    """jg_node_await."""
    _fields_ = [("attached", C.c_uint32), ("state", C.c_uint32), ("rows", C.c_void_p), ("rows_n", C.c_size_t), ("total", C.c_size_t),
                ("stats", AwaitStats), ("marked", C.c_size_t)]


NODE_LOOKUP_MAX = 65536  # jg_step_node_looked: the most entries a step can carry


class NodeLookup(C.Structure):
    """jg_node_lookup."""
    _fields_ = [("attached", C.c_uint32), ("state", C.c_uint32), ("rows", C.c_void_p), ("n", C.c_size_t), ("match", C.c_void_p)]


NODE_HOSTING_MAX = 65536  # jg_step_node_hosted: the most entries of a host list (or of self_slots) a step can carry
NODE_HOSTING_CLOSE_REFUSED, NODE_HOSTING_OPEN_REFUSED = 2, 4  # jg_node_hosting.state, beside NODE_POLL_REDONE


class NodeHostingRequest(C.Structure):
    """jg_node_hosting_request."""
    _fields_ = [("close", C.c_void_p), ("open", C.c_void_p)]


class NodeHosting(C.Structure):
    """jg_node_hosting."""
    _fields_ = [("attached", C.c_uint32), ("state", C.c_uint32), ("closed", C.c_uint32), ("opened", C.c_uint32)]


# mailbox words (josefine_gpu.h: JG_ANSWER / JG_AE)
MAILBOX_NONE = (1 << 56) - 1


def pack_answers(ack_head, hb_has):
    """JG_ANSWER: AppendResponse.head (NO_ACK: none) and the HeartbeatResponse code per entry."""
    import numpy as np
    a = np.asarray(ack_head, dtype=np.uint64)
    field = np.where(a == np.uint64(NO_ACK), np.uint64(MAILBOX_NONE), a)
    # (a head that does not fit 56 bits cannot be put on the wire: the engines fault where they produce one)
    return (field << np.uint64(8)) | np.asarray(hb_has, dtype=np.uint64)


def unpack_answers(words):
    import numpy as np
    w = np.asarray(words, dtype=np.uint64)
    field = w >> np.uint64(8)
    return np.where(field == np.uint64(MAILBOX_NONE), np.uint64(NO_ACK), field), (w & np.uint64(0xFF)).astype(np.uint8)


def pack_ae(ae_from, ae_n):
    import numpy as np
    n = np.asarray(ae_n, dtype=np.uint64)
    return np.where(n == np.uint64(AE_NONE), np.uint64(NO_ACK), (np.asarray(ae_from, dtype=np.uint64) << np.uint64(8)) | n)


def unpack_ae(words):
    import numpy as np
    w = np.asarray(words, dtype=np.uint64)
    n = (w & np.uint64(0xFF)).astype(np.uint8)
    return np.where(n == AE_NONE, np.uint64(0), w >> np.uint64(8)), n


# numpy structured dtypes matching jg_msg_row / jg_fsm_row / jg_fault_row
MSG_DTYPE = [("group", "<u4"), ("kind", "u1"), ("to_kind", "u1"), ("flag", "u1"), ("pad", "u1"),
             ("to_id", "<u4"), ("from", "<u4"), ("term", "<u8"), ("id", "<u8"), ("aux", "<u8")]
FSM_DTYPE = [("group", "<u4"), ("kind", "u1"), ("pad", "u1", (3,)), ("a", "<u8"), ("b", "<u8")]
FAULT_DTYPE = [("group", "<u4"), ("code", "<u4")]
COMPACT_DTYPE = [("group", "<u4"), ("pad", "<u4"), ("id", "<u8")]
LEADER_ROW_DTYPE = [("group", "<u4"), ("leader_id", "<u4"), ("term", "<u8"), ("role", "u1"), ("state", "u1"), ("fault", "u1"),
                    ("self_slot", "u1"), ("reserved", "<u4")]
ISR_ROW_DTYPE = [("group", "<u4"), ("isr", "u1"), ("replicate", "u1"), ("state", "u1"), ("self_slot", "u1"), ("head", "<u8"),
                 ("worst_lag", "<u8")]
# jg_group_state: a row of jg_engine_lookup_groups (80 bytes)
GROUP_STATE_DTYPE = [("group", "<u4"), ("known_leader", "<u4"), ("term", "<u8"), ("head", "<u8"), ("commit", "<u8"), ("id_gen", "<u8"),
                     ("election_time", "<u8"), ("heartbeat_time", "<u8"), ("voted_for", "<u4"), ("leader_id", "<u4"),
                     ("election_timeout", "<u4"), ("queued_reqs", "<u4"), ("role", "u1"), ("state", "u1"), ("fault", "u1"),
                     ("self_slot", "u1"), ("repl_state", "u1"), ("vote_seen", "u1"), ("vote_granted", "u1"), ("has", "u1")]
# jg_commit_row: a row of jg_engine_watch_commits (48 bytes)
COMMIT_ROW_DTYPE = [("group", "<u4"), ("role", "u1"), ("state", "u1"), ("fault", "u1"), ("self_slot", "u1"), ("term", "<u8"),
                    ("commit_from", "<u8"), ("commit", "<u8"), ("head_from", "<u8"), ("head", "<u8")]
# jg_await_row / jg_done_row: a waiter and a row of jg_engine_watch_completions (48 bytes each)
AWAIT_ROW_DTYPE = [("group", "<u4"), ("flags", "<u4"), ("token", "<u8"), ("block_id", "<u8"), ("term", "<u8"),
                   ("deadline_ms", "<u8"), ("reserved", "<u8")]
DONE_ROW_DTYPE = [("group", "<u4"), ("state", "u1"), ("role", "u1"), ("fault", "u1"), ("self_slot", "u1"), ("token", "<u8"),
                  ("block_id", "<u8"), ("term_now", "<u8"), ("commit_now", "<u8"), ("head_now", "<u8")]

_P = C.c_void_p


class Api:
    """Function table for one loaded library."""

    # name -> (restype, argtypes); names without prefix
    _PROTOS = {
        "engine_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
        "engine_destroy": (None, [_P]),
        "set_self_slots": (C.c_int, [_P, _P]),
        "submit": (C.c_int, [_P, C.POINTER(CmdBatch)]),
        "step": (C.c_int, [_P, C.c_uint64]),
        "step_dense_acks": (C.c_int, [_P, _P]),
        "step_dense_leader": (C.c_int, [_P, C.c_uint64, C.POINTER(LeaderInbox), C.POINTER(LeaderOutbox)]),
        "step_dense_follower": (C.c_int, [_P, C.c_uint64, C.POINTER(FollowerInbox), C.POINTER(FollowerOutbox), C.c_int]),
        "chain_compact": (C.c_int, [_P, C.c_size_t, _P, _P, _P, _P, _P]),
        "chain_compact_resident": (C.c_int, [_P, C.POINTER(C.c_size_t)]),
        "drain_compacted": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
        "drain_messages": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
        "drain_applies": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
        "drain_faults": (C.c_int, [_P, _P, C.c_size_t, C.POINTER(C.c_size_t)]),
        "read_state": (C.c_int, [_P, C.c_int, C.c_uint32, _P, C.c_uint32, C.c_uint32]),
        "get_counters": (C.c_int, [_P, C.POINTER(C.c_uint64 * 4)]),
        "last_error": (C.c_char_p, []),
        "abi_version": (C.c_uint32, []),
        "step_node": (C.c_int, [_P, C.c_uint64, C.c_uint32]),
        "node_outbox_view": (C.c_int, [_P, C.POINTER(NodeOutbox)]),
        "node_inbox_columns": (C.c_int, [_P, C.c_uint32, C.POINTER(_P), C.POINTER(_P)]),
    }
    # only the device engine has these
    _DEVICE_PROTOS = {
        "shard_count": (C.c_uint32, [_P]),
        "get_shard": (C.c_int, [_P, C.c_uint32, C.POINTER(ShardInfo)]),
        "step_dense_acks_shards": (C.c_int, [_P, C.POINTER(_P), C.c_uint32]),
        "step_device_rows": (C.c_int, [_P, C.POINTER(CmdBatch), C.c_uint64]),
        "step_dense_acks_device": (C.c_int, [_P, _P]),
        "step_dense_acks_device_n": (C.c_int, [_P, _P, C.c_uint32]),
        "sync": (C.c_int, [_P]),
        "stream_wait": (C.c_int, [_P, _P]),
        "drain_prefetch": (C.c_int, [_P]),
        "drain_flush": (C.c_int, [_P]),
        "drain_wait": (C.c_int, [_P]),
        "drain_messages_view": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
        "drain_applies_view": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
        "device_alloc": (C.c_int, [_P, C.c_size_t, C.POINTER(_P)]),
        "device_free": (C.c_int, [_P, _P]),
        "device_upload": (C.c_int, [_P, _P, _P, C.c_size_t]),
        "device_download": (C.c_int, [_P, _P, _P, C.c_size_t]),
        "timer_start": (C.c_int, [_P]),
        "timer_stop": (C.c_int, [_P, C.POINTER(C.c_float)]),
        "synth_fill_acks_device": (C.c_int, [_P, C.c_uint32, C.c_uint64, _P, _P]),
        "calibrate_stream": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_float)]),
        "submit_reserve": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.POINTER(CmdCols)]),
        "submit_commit": (C.c_int, [_P, C.c_size_t, C.c_size_t, C.c_uint32]),
        "dense_cluster_create": (C.c_int, [C.POINTER(_P), C.c_uint32, C.c_uint32, C.POINTER(_P)]),
        "dense_cluster_destroy": (None, [_P]),
        "dense_cluster_set_option": (C.c_int, [_P, C.c_uint32, C.c_uint64]),
        "dense_cluster_set_appends": (C.c_int, [_P, C.c_uint64, _P]),
        "dense_cluster_withdraw_appends": (C.c_int, [_P, _P, C.c_uint32]),
        "dense_cluster_offer_appends": (C.c_int, [_P, _P, C.c_uint32, C.c_uint64]),
        "dense_cluster_rounds": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_uint32]),
        "dense_cluster_mailboxes": (C.c_int, [_P, C.POINTER(LeaderInbox), C.POINTER(LeaderOutbox)]),
        "dense_cluster_round_routed": (C.c_int, [_P, C.c_uint64, C.POINTER(CmdBatch), C.POINTER(RouteStats)]),
        "kernel_timing": (C.c_int, [_P, C.c_int]),
        "kernel_timing_read": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
        "engine_load_chains": (C.c_int, [_P, C.c_uint64, C.POINTER(ChainImage)]),
        "engine_read_chains": (C.c_int, [_P, C.POINTER(ChainRead), C.POINTER(C.c_uint64)]),
        "engine_export_groups": (C.c_int, [_P, C.POINTER(GroupExport)]),
        "engine_import_groups": (C.c_int, [_P, C.POINTER(GroupImport)]),
        "engine_open_groups": (C.c_int, [_P, C.c_uint64, C.POINTER(GroupSet)]),
        "engine_close_groups": (C.c_int, [_P, C.POINTER(GroupSet)]),
        "engine_list_groups": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
        "engine_watch_leaders": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
        "engine_census": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(Census)]),
        "engine_watch_replicas": (C.c_int, [_P, C.c_uint32, C.POINTER(IsrPolicy), C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_size_t)]),
        "engine_replication_census": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(ReplCensus)]),
        "engine_watch_replicas_timed": (C.c_int, [_P, C.c_uint32, C.POINTER(IsrClock), C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t,
                                                  C.POINTER(C.c_size_t)]),
        "engine_lookup_groups": (C.c_int, [_P, C.POINTER(GroupSet), C.c_void_p, C.c_void_p]),
        "engine_watch_commits": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                           C.POINTER(CommitBacklog)]),
        "engine_await_open": (C.c_int, [_P, C.c_size_t]),
        "engine_await_blocks": (C.c_int, [_P, C.c_void_p, C.c_size_t]),
        "engine_watch_completions": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                               C.POINTER(AwaitStats)]),
        "engine_await_cancel": (C.c_int, [_P, C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(C.c_size_t)]),
        "engine_poll": (C.c_int, [_P, C.POINTER(Poll)]),
        "step_node_polled": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.POINTER(Poll)]),
        "node_poll_view": (C.c_int, [_P, C.POINTER(NodePoll)]),
        "step_node_awaited": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.POINTER(Poll), C.POINTER(NodeAwaitRequest)]),
        "node_await_view": (C.c_int, [_P, C.POINTER(NodeAwait)]),
        "step_node_looked": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.POINTER(Poll), C.POINTER(NodeAwaitRequest), C.POINTER(GroupSet)]),
        "node_lookup_view": (C.c_int, [_P, C.POINTER(NodeLookup)]),
        "step_node_hosted": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.POINTER(Poll), C.POINTER(NodeAwaitRequest), C.POINTER(GroupSet),
                                       C.POINTER(NodeHostingRequest)]),
        "node_hosting_view": (C.c_int, [_P, C.POINTER(NodeHosting)]),
    }
    # only the oracle has these
    _ORACLE_PROTOS = {
        "set_threads": (C.c_int, [_P, C.c_uint]),
        "synth_fill_acks": (C.c_int, [_P, C.c_uint32, C.c_uint64, _P, _P]),
    }

    def __init__(self, path: str, prefix: str):
        self.path = path
        self.prefix = prefix
        self.lib = C.CDLL(path, mode=C.RTLD_GLOBAL if False else C.RTLD_LOCAL)
        for table, required in ((self._PROTOS, True), (self._DEVICE_PROTOS, False), (self._ORACLE_PROTOS, False)):
            for name, (res, args) in table.items():
                sym = prefix + name
                try:
                    fn = getattr(self.lib, sym)
                except AttributeError:
                    if required:
                        raise ImportError(f"{path} does not export {sym}")
                    continue
                fn.restype = res
                fn.argtypes = args
                setattr(self, name, fn)

    def exported(self, name: str) -> bool:
        return hasattr(self.lib, self.prefix + name)

    def error(self) -> str:
        msg = self.last_error()
        return msg.decode() if msg else ""


# Every symbol include/josefine_gpu.h declares (checked by the CPU test-suite).
HEADER_SYMBOLS = [
    "jg_engine_create", "jg_engine_destroy", "jg_shard_count", "jg_get_shard", "jg_step_dense_acks_shards", "jg_set_self_slots", "jg_submit", "jg_step", "jg_step_device_rows",
    "jg_step_dense_acks", "jg_step_dense_acks_device", "jg_step_dense_acks_device_n",
    "jg_step_dense_leader", "jg_step_dense_follower", "jg_chain_compact", "jg_chain_compact_resident", "jg_drain_compacted", "jg_sync", "jg_stream_wait",
    "jg_drain_messages", "jg_drain_applies", "jg_drain_faults", "jg_drain_messages_view", "jg_drain_applies_view", "jg_drain_prefetch", "jg_drain_flush", "jg_drain_wait", "jg_read_state", "jg_get_counters",
    "jg_device_alloc", "jg_device_free", "jg_device_upload", "jg_device_download",
    "jg_timer_start", "jg_timer_stop", "jg_synth_fill_acks_device", "jg_calibrate_stream", "jg_dense_cluster_create", "jg_dense_cluster_destroy", "jg_dense_cluster_set_option", "jg_dense_cluster_set_appends", "jg_dense_cluster_withdraw_appends", "jg_dense_cluster_offer_appends", "jg_dense_cluster_rounds", "jg_dense_cluster_mailboxes", "jg_dense_cluster_round_routed", "jg_kernel_timing", "jg_kernel_timing_read", "jg_last_error", "jg_abi_version",
    "jg_step_node", "jg_node_outbox_view", "jg_submit_reserve", "jg_submit_commit", "jg_node_inbox_columns",
    "jg_engine_load_chains", "jg_engine_read_chains", "jg_engine_export_groups", "jg_engine_import_groups",
    "jg_engine_open_groups", "jg_engine_close_groups", "jg_engine_list_groups",
    "jg_engine_watch_leaders", "jg_engine_census",
    "jg_engine_watch_replicas", "jg_engine_replication_census",
    "jg_engine_lookup_groups",
    "jg_engine_watch_commits",
    "jg_engine_poll",
    "jg_step_node_polled", "jg_node_poll_view",
    "jg_engine_watch_replicas_timed",
    "jg_engine_await_open", "jg_engine_await_blocks", "jg_engine_watch_completions",
    "jg_step_node_awaited", "jg_node_await_view",
    "jg_engine_await_cancel",
    "jg_step_node_looked", "jg_node_lookup_view",
    "jg_step_node_hosted", "jg_node_hosting_view",
]
