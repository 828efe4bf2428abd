/*
 * josefine_gpu.h — C ABI of the MI355X batched Chained-Raft engine.
 *
 * This is the drop-in boundary for the hot path of tychedelia/josefine's
 * `src/raft` state machine.  One engine hosts N independent
 * Raft node instances ("groups", index g) and applies batches of
 * `Command`s to them with exactly the per-instance semantics of the reference's
 *
 *     trait Apply { fn apply(self, cmd: Command) -> Result<RaftHandle>; }
 *                                               (src/raft/mod.rs:483-489)
 *
 * Plain pointers and sizes only: this header is what a Rust `extern "C"`
 * block / bindgen would bind (see INTEGRATION.md for the adapter that
 * implements `Apply` on top of it).  All paths cited below are relative to the
 * reference checkout.
 *
 * Conventions
 *   - every entry point returns 0 (JG_OK) or a negative JG_E* status;
 *     `jg_last_error()` returns a thread-local description of the last failure;
 *   - reference panics / `Err` returns never abort a batch: they are recorded as
 *     a sticky per-group fault code (`JG_FIELD_FAULT`), after which the group
 *     ignores commands until `JG_CMD_RESTART` (the process would be dead) - a
 *     vacant slot (`JG_FAULT_VACANT`) ignores those too, until it is opened;
 *   - BlockId is the reference's 8-byte big-endian id (src/raft/chain.rs:29-36,
 *     63-67) carried as a native uint64_t (same ordering);
 *   - one engine is externally synchronised (one caller thread at a time),
 *     exactly like the by-value `RaftHandle` (src/raft/mod.rs:471-479).
 */
#ifndef JOSEFINE_GPU_H
#define JOSEFINE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JG_ABI_VERSION 26u /* v26: jg_step_node_hosted / jg_node_hosting_view, JG_NODE_HOSTING_MAX (opening and closing partitions behind a kept node step: LeaderAndIsr with two ticks in flight); v25: jg_step_node_looked / jg_node_lookup_view, JG_NODE_LOOKUP_MAX (point queries behind a kept node step: Metadata with two ticks in flight); v24: jg_engine_await_cancel, jg_node_await_request.cancel_keys / cancel_n / cancel_mask, jg_node_await.marked, JG_DONE_CANCELLED (withdrawing waiters: a closed connection leaves the purgatory); v23: jg_step_node_awaited / jg_node_await_view (completions behind a kept node step: the purgatory with two ticks in flight); v22: jg_engine_await_open / jg_engine_await_blocks / jg_engine_watch_completions (the completion feed: fsm::Driver's notifications on the device); v21: jg_step_node_polled / jg_node_poll_view (a poll behind a kept node step: the feeds with two ticks in flight); v20: jg_poll.clock (jg_engine_poll answers the replicas part under the time rule: the clocks advance in the one fused pass); v19: jg_engine_watch_replicas_timed (time-based in-sync sets: a per-replica clock in the replication feed); v18: jg_engine_poll (one poll per tick: the three change feeds and the two censuses in one call, one pass and one synchronisation); v17: jg_engine_watch_commits (the commit feed: what dense steps committed and appended); v16: jg_engine_lookup_groups (point queries: the state of a list of partitions in one call); v15: jg_engine_watch_replicas / jg_engine_replication_census (the replication feed: in-sync sets on the device); v14: jg_engine_watch_leaders / jg_engine_census (the leadership feed and the census); v13: vacant slots - jg_engine_open_groups / jg_engine_close_groups / jg_engine_list_groups, JG_CFG_START_VACANT, JG_FAULT_VACANT; v12: jg_engine_export_groups / jg_engine_import_groups (live groups handed between engines); v11: jg_engine_read_chains (the chain trees read back out, the inverse of v10); v10: jg_engine_load_chains (an engine opened on persisted chain trees); v9: JG_NODE_KEEP (two node steps in flight: jg_node_outbox_view serves the oldest); v8: jg_dense_cluster_round_routed delivers a partition's mail in the order (phase, emission index, sender) instead of
                             (sender, step, emission index) - same entry points, same layouts, different (legal) network schedule; v5: jg_step_node = arrival-order Apply (fsm_tx: Apply / Notify / Apply per partition), JG_CLUSTER_ANY_LEADER,
                             jg_dense_cluster_withdraw_appends, JG_COL_UNCHECKED, JG_COL_UPLOAD_NOW; v6: jg_dense_cluster_set_option, jg_dense_cluster_offer_appends, JG_CMD_RECREATE;
                             v7: the node step's bus formats - JG_COL_PACKED_KIND, JG_COL_ID32, JG_NODE_COMMON_AE (jg_node_outbox.aec), JG_NODE_FSM_FUSED (JG_FSM_LEADER_STEP) */
#define JG_MAX_REPLICAS 8u  /* R <= 8: vote / progress-state masks are one byte            */
#define JG_CHAIN_WINDOW 8u  /* chain segments (gaps / forks) per group besides the main run */
#define JG_MAX_INFLIGHT 5u  /* src/raft/progress.rs:117                                    */
#define JG_FOREIGN_VOTERS 8u /* distinct voters outside the membership an election remembers */
#define JG_NO_ACK UINT64_MAX /* dense ack column: "no AppendResponse from this replica"    */
#define JG_MAX_DEVICES 16u  /* shards (devices) behind one engine handle                      */
#define JG_MAX_DENSE_APPENDS (1u << 20) /* own slot of a dense ack block: appends per group per tick */

/* ---- status codes -------------------------------------------------------- */
enum {
  JG_OK = 0,
  JG_EINVAL = -1,   /* bad argument / config (cf. RaftConfig::validate, src/raft/config.rs:60-84) */
  JG_ENOMEM = -2,
  JG_EDEVICE = -3,  /* HIP runtime error; no CPU fallback exists                    */
  JG_ECAPACITY = -4 /* caller's output buffer too small; nothing was consumed       */
};

/* ---- roles: RaftHandle variants, src/raft/mod.rs:417-425 ------------------ */
enum { JG_ROLE_FOLLOWER = 0, JG_ROLE_CANDIDATE = 1, JG_ROLE_LEADER = 2 };

/* ---- Command kinds: enum Command, src/raft/mod.rs:160-227 ------------------
 * Column use per kind (unused columns are ignored):
 *   kind              from          term   id            aux        flag
 *   TICK              -             -      -             -          -
 *   PROPOSE           -             -      -             -          -
 *   VOTE_REQUEST      candidate_id  term   head          last_term  -
 *   VOTE_RESPONSE     from          term   -             -          granted
 *   APPEND_ENTRIES    leader_id     term   first block*  n_blocks   -
 *   APPEND_RESPONSE   node_id       term   head          -          success
 *   HEARTBEAT         leader_id     term   commit        -          -
 *   HEARTBEAT_RESPONSE (sender**)   -      commit        -          has_committed
 *   TIMEOUT           -             -      -             -          -
 *   NOOP              -             -      -             -          -
 *   CLIENT_REQUEST    -             -      request token -          -
 *   CLIENT_RESPONSE   -             -      request token -          -
 *   RESTART (engine)  -             -      -             -          -
 *   RECREATE (engine) -             -      -             -          -
 * (*) index of the first of `aux` consecutive entries in the batch's
 *     blk_id/blk_next side arrays (Vec<Block>, payload stays on the host).
 * (**) the reference's handler does not look at the sender (leader.rs:222-231) and neither does
 *     jg_step; jg_step_node needs Message.from (rpc.rs:17-27) to put the response into the
 *     sender's mailbox slot (0 or a non-member: the row takes the general path).
 * RESTART is not a reference Command: it restates process restart, i.e.
 * `Raft::<Follower>::new` + `Chain::new` on the persisted tree
 * (src/raft/follower.rs:68-95, src/raft/chain.rs:117-137), and clears the fault.
 */
enum {
  JG_CMD_TICK = 0,
  JG_CMD_PROPOSE = 1,
  JG_CMD_VOTE_REQUEST = 2,
  JG_CMD_VOTE_RESPONSE = 3,
  JG_CMD_APPEND_ENTRIES = 4,
  JG_CMD_APPEND_RESPONSE = 5,
  JG_CMD_HEARTBEAT = 6,
  JG_CMD_HEARTBEAT_RESPONSE = 7,
  JG_CMD_TIMEOUT = 8,
  JG_CMD_NOOP = 9,
  JG_CMD_CLIENT_REQUEST = 10,
  JG_CMD_CLIENT_RESPONSE = 11,
  JG_CMD_RESTART = 12,
  JG_CMD_RECREATE = 13,
  JG_CMD__COUNT = 14
};
/* The two engine commands (no reference Command): JG_CMD_RESTART = the replica's process restarts on its persisted tree
 * (Raft::new + Chain::new on the sled directory it left: follower.rs:68-95, chain.rs:117-137); JG_CMD_RECREATE = on an
 * EMPTY directory - the replica of a partition that was re-created: genesis only, no "commit" key (chain.rs:117-153), and
 * the host's block store for the group starts over with it.  Both clear a fault; neither looks at the other columns. */

/* ---- Address, src/raft/rpc.rs:5-14 ---------------------------------------- */
enum { JG_TO_PEERS = 0, JG_TO_PEER = 1, JG_TO_LOCAL = 2, JG_TO_CLIENT = 3, JG_TO_QUEUE = 4 };

/* ---- client request queue rows ----------------------------------------------
 * Follower / Candidate queue client requests they cannot forward yet
 * (src/raft/follower.rs:22,258-270; candidate.rs:20,190-193).  The request
 * payloads stay with the host adapter; the engine keeps only the queue length
 * and tells the adapter what to do with its mirror through CLIENT_REQUEST rows:
 *   to_kind JG_TO_QUEUE, flag 0              : push request `id` onto the group's queue
 *   to_kind JG_TO_PEER,  flag JG_QUEUE_FLUSH : send the `aux` queued requests, in order, to
 *                                              to_id, then clear the queue (follower.rs:190-197)
 *   to_kind JG_TO_QUEUE, flag JG_QUEUE_DROP  : the `aux` queued requests are dropped by a
 *                                              role change (follower.rs:295, candidate.rs:216-238)
 *   to_kind JG_TO_PEER,  flag 0              : forward request `id` now (follower.rs:262-265) */
enum { JG_QUEUE_FLUSH = 1, JG_QUEUE_DROP = 2 };

/* ---- fault codes ------------------------------------------------------------
 * 1..63: the reference would panic or return Err at the cited line.
 * 128.. : engine-domain limits (inputs outside what the device layout can
 *         represent); never silently wrong, always loud. */
enum {
  JG_FAULT_NONE = 0,
  JG_FAULT_LEADER_TERM_UNIMPLEMENTED = 1, /* leader.rs:33-35 via leader.rs:200-208, mod.rs:360-365 */
  JG_FAULT_APPEND_ID_NOT_ABOVE_HEAD = 2,  /* chain.rs:163 assert!(id > self.head)                  */
  JG_FAULT_PROGRESS_UNKNOWN_NODE = 3,     /* progress.rs:43 expect("the node does not exist")      */
  JG_FAULT_COMMIT_MISSING_BLOCK = 4,      /* chain.rs:197-202 panic!("")                           */
  JG_FAULT_EXTEND_MISSING_PARENT = 5,     /* chain.rs:180-185 Err via follower.rs:159              */
  JG_FAULT_FOLLOWER_STALE_LEADER = 6,     /* follower.rs:147-154 assert!                           */
  JG_FAULT_CANDIDATE_TICK_ELECTED = 7,    /* candidate.rs:64 panic!("this should never happen")    */
  JG_FAULT_RANGE_HIT_COMMIT_KEY = 8,      /* chain.rs:198 + 219-226 via leader.rs:135,152-157 (Q9) */
  JG_FAULT_ENGINE_WINDOW_OVERFLOW = 128,  /* chain needs > JG_CHAIN_WINDOW segments (gaps / forks) */
  JG_FAULT_ENGINE_FOREIGN_VOTER = 129,    /* a 9th distinct voter outside the membership in one election
                                             (the first JG_FOREIGN_VOTERS are counted, election.rs:33-35) */
  JG_FAULT_ENGINE_DENSE_NONLEADER = 131,  /* dense tick asked a non-leader group to append         */
  JG_FAULT_ENGINE_DENSE_APPENDS = 132,    /* own slot of a dense ack block >= JG_MAX_DENSE_APPENDS */
  JG_FAULT_ENGINE_MAILBOX_RANGE = 133,    /* a block id >= 2^56 - 1 would have to go into a mailbox word */
  JG_FAULT_VACANT = 255                   /* not a fault: the slot hosts no partition (jg_engine_close_groups) */
};

/* ---- engine configuration ---------------------------------------------------
 * Restates the parts of RaftConfig that feed L1 (src/raft/config.rs:14-41,
 * defaults 87-111) for N instances at once.  `node_ids[r]` is the NodeId of
 * replica slot r; an instance's own slot is `self_slot[g]` (default 0) and its
 * `config.nodes` are the other slots in ascending slot order. */
typedef struct jg_config {
  uint32_t abi_version;              /* JG_ABI_VERSION                                        */
  uint32_t n_groups;                 /* G                                                     */
  uint32_t n_replicas;               /* R = config.nodes.len()+1, 1..JG_MAX_REPLICAS          */
  uint32_t node_ids[JG_MAX_REPLICAS];/* nonzero, distinct (config.rs:64-66)                   */
  int32_t device_id;                 /* HIP device ordinal                                    */
  uint32_t heartbeat_timeout_ms;     /* config.rs:104 (100)                                   */
  uint32_t election_timeout_min_ms;  /* mod.rs:318 (500)                                      */
  uint32_t election_timeout_max_ms;  /* mod.rs:319 (1000)                                     */
  uint64_t seed;                     /* replaces thread_rng (follower.rs:105); see DESIGN.md  */
  uint64_t group_base;               /* global id of local group 0 (sharding; keys the RNG)   */
  uint32_t flags;                    /* JG_CFG_*                                              */
  uint32_t reserved;
  /* Multi-device engine (SURVEY.md §8(b),(e)): n_devices >= 1 shards the G groups over
   * device_ids[0..n_devices) by contiguous ownership — shard d owns local groups
   * [d*S, min((d+1)*S, G)) with S = ceil(G / n_devices) (trailing shards that would be empty are
   * not created) — behind this ONE handle: the reference has one caller that owns the handle
   * (event_loop, src/raft/server.rs:103-165).  A device may be listed more than once (several
   * shards on one GPU).  n_devices == 0: one shard on `device_id`. */
  uint32_t n_devices;
  int32_t device_ids[JG_MAX_DEVICES];
} jg_config;

enum {
  /* keep the "commit" key out of the block keyspace, i.e. do NOT reproduce Q9
   * (SURVEY.md §7.3): unbounded ranges then simply end at the last block. */
  JG_CFG_SEPARATE_COMMIT_KEY = 1u,
  /* jg_step_node's row passes UNTILED: one thread per row scatters into the G-sized columns (three random 4-8-byte
   * accesses per row and pass) instead of binning the rows by tile of 256 partitions and applying a tile's rows to its
   * columns in LDS.  The results are the same bit for bit; the flat passes are the statement the tiled ones are held to
   * (tests/test_node_step.py) and an A/B switch - nothing to set in production. */
  JG_CFG_FLAT_ROW_PASSES = 2u,
  /* every slot starts VACANT (jg_engine_open_groups): a broker sizes the engine's capacity, then opens partitions */
  JG_CFG_START_VACANT = 4u
};

/* ---- SoA command batch (host memory), SURVEY.md §8(a) a18 -------------------- */
typedef struct jg_cmd_batch {
  size_t n;               /* number of command rows                                       */
  const uint8_t* kind;    /* [n] JG_CMD_*                                                 */
  const uint32_t* group;  /* [n] local group index; rows of one group apply in row order  */
  const uint32_t* from;   /* [n] NodeId                                                   */
  const uint64_t* term;   /* [n]                                                          */
  const uint64_t* id;     /* [n] BlockId / token / side-array index                       */
  const uint64_t* aux;    /* [n]                                                          */
  const uint8_t* flag;    /* [n]                                                          */
  size_t n_blocks;        /* entries in the side arrays                                   */
  const uint64_t* blk_id; /* [n_blocks] Block.id   (chain.rs:86-91)                       */
  const uint64_t* blk_next;/*[n_blocks] Block.next                                        */
} jg_cmd_batch;

/* ---- outbound Message rows: what the reference pushes on rpc_tx -----------
 * (src/raft/mod.rs:337-340,390-400; src/raft/rpc.rs:17-27).  `kind` is the
 * Command kind; columns as in the table above, with `from` = sender NodeId.
 * APPEND_ENTRIES rows (leader.rs:124-174) carry id = range start key
 * (progress.head) and aux = number of blocks: the payload is the next `aux`
 * stored blocks after skipping the first item of `range(id..)`. */
typedef struct jg_msg_row {
  uint32_t group;
  uint8_t kind;
  uint8_t to_kind; /* JG_TO_* */
  uint8_t flag;
  uint8_t pad;
  uint32_t to_id;  /* NodeId when to_kind == JG_TO_PEER */
  uint32_t from;
  uint64_t term;
  uint64_t id;
  uint64_t aux;
} jg_msg_row;

/* ---- FSM instruction rows: what the reference pushes on fsm_tx -------------
 * (src/raft/fsm.rs:20-29).  Apply instructions are run-length encoded as key
 * ranges; the host expands them against its block store in key order:
 *   JG_FSM_APPLY_LEADER   : range(a..=b).skip(1)   (leader.rs:93)
 *   JG_FSM_APPLY_FOLLOWER : range(a..b)            (follower.rs:204, half-open)
 *   JG_FSM_NOTIFY         : Notify{block_id=a, id=b} (leader.rs:184-188)
 *   JG_FSM_LEADER_STEP    : (jg_step_node with JG_NODE_FSM_FUSED only) everything a leader partition pushed in
 *                           one step as ONE row: a = the appended block's id, b = the ClientRequest's token,
 *                           pad[0..2] = a - c0, a - c1, a - c2 (each <= 255) standing for, in this order,
 *                             JG_FSM_APPLY_LEADER {c0, c1} if c1 != c0;  JG_FSM_NOTIFY {a, b};
 *                             JG_FSM_APPLY_LEADER {c1, c2} if c2 != c1 */
enum { JG_FSM_APPLY_LEADER = 0, JG_FSM_APPLY_FOLLOWER = 1, JG_FSM_NOTIFY = 2, JG_FSM_LEADER_STEP = 3 };
typedef struct jg_fsm_row {
  uint32_t group;
  uint8_t kind;
  uint8_t pad[3];
  uint64_t a;
  uint64_t b;
} jg_fsm_row;

typedef struct jg_fault_row {
  uint32_t group;
  uint32_t code; /* JG_FAULT_* */
} jg_fault_row;

/* ---- state columns readable through jg_read_state ------------------------- */
enum {
  JG_FIELD_TERM = 0,        /* u64  State.current_term          mod.rs:277            */
  JG_FIELD_VOTED_FOR = 1,   /* u32  State.voted_for or 0        mod.rs:279            */
  JG_FIELD_HAS_VOTED = 2,   /* u8   voted_for.is_some()                                */
  JG_FIELD_ROLE = 3,        /* u8   JG_ROLE_*                   mod.rs:417-425        */
  JG_FIELD_COMMIT = 4,      /* u64  Chain.commit                chain.rs:102          */
  JG_FIELD_HEAD = 5,        /* u64  Chain.head                  chain.rs:103          */
  JG_FIELD_ID_GEN = 6,      /* u64  Chain.id_gen                chain.rs:101          */
  JG_FIELD_MATCH = 7,       /* u64  Progress.head of `replica`  progress.rs:124       */
  JG_FIELD_REPL_STATE = 8,  /* u8   bit r = Replicate (else Probe) progress.rs:62-66  */
  JG_FIELD_VOTE_SEEN = 9,   /* u8   bit r = votes.contains(r)   election.rs:8         */
  JG_FIELD_VOTE_GRANTED = 10,/*u8   bit r = votes[r] == true                           */
  JG_FIELD_FAULT = 11,      /* u8   JG_FAULT_*                                         */
  JG_FIELD_LEADER_ID = 12,  /* u32  Follower.leader_id or 0     follower.rs:20        */
  JG_FIELD_HAS_LEADER = 13, /* u8                                                      */
  JG_FIELD_ELECTION_TIME = 14,   /* u64 ms, State.election_time       mod.rs:281      */
  JG_FIELD_ELECTION_TIMEOUT = 15,/* u32 ms, State.election_timeout    mod.rs:283      */
  JG_FIELD_HEARTBEAT_TIME = 16,  /* u64 ms, Leader.heartbeat_time     leader.rs:27    */
  JG_FIELD_QUEUED_REQS = 17,     /* u32 queued_reqs.len()  follower.rs:22, candidate.rs:20 */
  JG_FIELD_SELF_SLOT = 18,  /* u8                                                      */
  JG_FIELD__COUNT = 19
};

typedef struct jg_engine jg_engine;

/* RaftHandle::new for every group (src/raft/mod.rs:428-435 -> follower.rs:68-95):
 * Follower, State::default(), fresh Chain (genesis block 0), election timer armed
 * at now = 0.  Fails with JG_EDEVICE when no gfx950 device / HIP runtime is usable. */
int jg_engine_create(const jg_config* cfg, jg_engine** out);
void jg_engine_destroy(jg_engine* e);

/* ---- startup on persisted trees (ABI v10) ---------------------------------------------------------
 * What a josefine broker does when its process starts: Raft::<Follower>::new for every partition,
 * which calls Chain::new on the sled tree the previous process left in config.data_directory
 * (src/raft/follower.rs:68-95, src/raft/chain.rs:117-137).  The image is a sled scan, verbatim, in
 * host memory: group g0 + i owns the blocks off[i] .. off[i + 1] - 1 (the CSR shape of
 * jg_chain_compact), ids STRICTLY ascending within a group (sled's order of the 8-byte big-endian
 * keys = numeric order), and the value of its "commit" key where has_commit[i] is 1.  Payloads stay
 * on the host.  Per group of the range:
 *   - its id set and parent pointers become exactly the image's blocks, its commit-key bit has_commit[i];
 *   - then what a JG_CMD_RESTART row does: Follower, term 0, no vote, no leader, empty queue, votes
 *     cleared, heartbeat_time 0; Chain::new (Q8): commit = head = id_gen = c (c = the commit key's
 *     value, else 0; c == 0 re-inserts genesis and id_gen is 1); the election timer re-armed at
 *     now_ms with the group's next RNG draw; the sticky fault cleared;
 *   - engine-domain limits become the group's sticky fault (jg_drain_faults), as a restart's would:
 *     more than JG_CHAIN_WINDOW segments besides the run, or a stored block 0 whose next is not 0
 *     (genesis' parent is implicit): JG_FAULT_ENGINE_WINDOW_OVERFLOW.
 * Groups outside [g0, g0 + n) are untouched: a fresh engine followed by a load of [0, G) is a process
 * that started on those trees.  The chains are held in the canonical form jg_chain_normalize leaves
 * (the run from genesis, each further segment a maximal stretch with next == id - 1), so the dense
 * paths take loaded groups as they take built ones.  JG_EINVAL, and nothing changes, for a malformed
 * image (off[0] != 0, off not monotone, the range outside G, ids not strictly ascending within a
 * group), for commands submitted and not yet stepped, and while kept node steps (JG_NODE_KEEP) are
 * outstanding.  A multi-device handle splits the range by group_lo; each shard loads its part on its
 * own device.  Loading into an engine that is a node of a jg_dense_cluster between rounds is the
 * caller's responsibility (the cluster's other nodes are not told). */
typedef struct jg_chain_image {
  uint32_t g0, n;             /* local groups [g0, g0 + n)                                     */
  const uint64_t* off;        /* [n + 1] CSR offsets into the block arrays, off[0] == 0         */
  const uint64_t* blk_id;     /* ids of group g0 + i: off[i] .. off[i + 1] - 1, strictly ascending */
  const uint64_t* blk_next;   /* Block.next of each                                             */
  const uint64_t* commit;     /* [n] value of the "commit" key (ignored where absent)           */
  const uint8_t* has_commit;  /* [n] 1 = the tree has a "commit" key                            */
} jg_chain_image;
int jg_engine_load_chains(jg_engine* e, uint64_t now_ms, const jg_chain_image* img);

/* ---- reading the trees back (ABI v11) --------------------------------------------------------------
 * The inverse of jg_engine_load_chains: what a sled scan of each group's tree would return, written
 * in host memory in the image's own CSR shape - group g0 + i owns the rows off[i] .. off[i + 1] - 1,
 * ids strictly ascending (sled's key order), each with its Block.next, and the value of its "commit"
 * key where has_commit[i] is 1 (commit[i] is 0 where the key is absent).  With from == NULL every
 * output but fault[] is exactly a jg_chain_image: loading it into a fresh engine gives each group
 * what a JG_CMD_RESTART row does on the original.  With from != NULL group g0 + i reports only the
 * block keys >= from[i] (Chain::range(from..), src/raft/chain.rs:208-228); the commit key is always
 * reported.  Per group:
 *   - the chain is decoded from whatever form it is held in (the implicit run of RUN / FAST chains,
 *     no run under JGF_NO_GENESIS, window segments in any order, a leader's lag-packed commit);
 *   - fault[i] is the group's sticky fault code.  Below 128 the reference panicked: the tree is
 *     reported as it stood at the panic.  From 128 on (engine-domain limits, e.g.
 *     JG_FAULT_ENGINE_WINDOW_OVERFLOW) the image is no longer the tree: the group reports 0 rows
 *     and has_commit[i] = 0.
 * The read changes nothing and reflects every step issued before it (JG_NODE_ASYNC steps are
 * settled first); commands submitted and not yet stepped are not in it.  JG_EINVAL for the range
 * outside G, a null argument, and while kept node steps (JG_NODE_KEEP) are outstanding.  *n_rows is
 * set to the number of rows; if it exceeds cap the call returns JG_ECAPACITY and writes nothing else
 * (cap = 0 with blk_id = blk_next = NULL is the sizing call).  Reading a node of a jg_dense_cluster
 * between rounds is allowed.  A multi-device handle sizes every shard before any output is
 * written, then concatenates the shards' parts. */
typedef struct jg_chain_read {
  uint32_t g0, n;           /* local groups [g0, g0 + n)                                          */
  const uint64_t* from;     /* [n] or NULL: rows are the block keys >= from[i]; NULL = the whole tree */
  uint64_t cap;             /* rows blk_id / blk_next can hold                                    */
  uint64_t* off;            /* [n + 1] out, off[0] == 0                                           */
  uint64_t* blk_id;         /* [cap] out: ids of group g0 + i at off[i] .. off[i + 1] - 1, ascending */
  uint64_t* blk_next;       /* [cap] out: Block.next of each                                      */
  uint64_t* commit;         /* [n] out: value of the "commit" key (0 where absent)                */
  uint8_t* has_commit;      /* [n] out                                                            */
  uint8_t* fault;           /* [n] out: the group's sticky fault code                             */
} jg_chain_read;
int jg_engine_read_chains(jg_engine* e, jg_chain_read* r, uint64_t* n_rows);

/* ---- handing live groups over (ABI v12) -----------------------------------------------------------
 * A lossless hand-over of groups between engines of ONE node (another device of the process, another
 * process on the same broker): jg_engine_export_groups writes a full-fidelity state image of local
 * groups [g0, g0 + n) - a header plus one fixed-stride record per group holding every column the
 * group's behaviour depends on (term, chain, commit, progress, timers, votes, role, fault; the layout
 * is DESIGN.md "Handing groups over") - and jg_engine_import_groups makes local groups
 * [g0, g0 + n) of another engine continue them bit for bit: no restart, no election.  Unlike
 * jg_engine_load_chains(jg_engine_read_chains(...)) the group keeps its leadership, its vote, its
 * replication progress and its election timer.
 *   - records live in host memory, or with JG_MOVE_DEVICE in device memory of the engine's own device
 *     (jg_device_alloc: 16-byte aligned); a multi-device parent handle takes the host form only.
 *   - the export changes nothing (JG_NODE_ASYNC steps are settled first, kept node steps refuse).
 *     With cap_bytes < n * record_bytes it fills the header, returns JG_ECAPACITY and writes nothing
 *     else (cap_bytes = 0 with records = NULL is the sizing call).  Output rows the groups already
 *     produced stay in the source's drains; jg_engine_close_groups (ABI v13) then makes the source's
 *     slots vacant, so that nothing drives them there any more.
 *   - the import adds shift_ms (wrapping u64) to every election_time and heartbeat_time: a destination
 *     driven at now + shift_ms decides as the source at now.  Future election timeouts are drawn under
 *     the destination's seed and global id (group_base + local; the draw count travels).
 *   - the import refuses with JG_EINVAL and writes nothing for: a range outside G or a null argument;
 *     a format or record_bytes mismatch; n_replicas, node_ids or the JG_CFG_SEPARATE_COMMIT_KEY bit
 *     differing from the destination's; queued commands; kept node steps; any record whose check word
 *     fails or whose fields are out of range (role, own slot >= R, window count > JG_CHAIN_WINDOW) -
 *     every record is validated on the device before the pass that writes (which also asserts that no
 *     per-step deferral state of the destination groups is pending: JG_EDEVICE if it is).  An imported group that
 *     carries a sticky fault writes no fault row (the source reported it).  Importing into a node of a
 *     jg_dense_cluster between rounds is allowed; the cluster's mailboxes are the caller's business.
 *   - extra device memory: a host-form export stages through two buffers of at most 2^18 records each
 *     (kept by the engine, shared with jg_engine_read_chains); a host-form import uploads the whole
 *     image first: n * record_bytes of scratch for the call.
 *   - a multi-device handle splits both calls by shard; an import checks every shard's refusals and
 *     validates every shard's records before any shard writes. */
#define JG_MOVE_FORMAT 1u  /* jg_group_image_header.format                                          */
#define JG_MOVE_DEVICE 1u  /* flags: the records are in device memory of the engine's device     */
typedef struct jg_group_image_header {
  uint32_t format;                    /* JG_MOVE_FORMAT                                       */
  uint32_t record_bytes;              /* stride of a record: a multiple of 64, fixed by R     */
  uint32_t n;                         /* records                                              */
  uint32_t n_replicas;                /* R of the source                                      */
  uint32_t node_ids[JG_MAX_REPLICAS]; /* the source's slots (must mean the same nodes)        */
  uint32_t separate_commit_key;       /* the source's JG_CFG_SEPARATE_COMMIT_KEY bit (0 / 1)   */
  uint32_t reserved;
  uint64_t seed;                      /* for information: the source's seed ...               */
  uint64_t global0;                   /* ... and the global id (group_base + local) of record 0 */
} jg_group_image_header;
typedef struct jg_group_export {
  uint32_t g0, n;                     /* local groups [g0, g0 + n)                            */
  uint32_t flags;                     /* JG_MOVE_DEVICE or 0                                  */
  uint32_t reserved;
  uint64_t cap_bytes;                 /* bytes `records` can hold                             */
  void* records;                      /* out: n records of header.record_bytes                */
  jg_group_image_header header;       /* out                                                  */
} jg_group_export;
typedef struct jg_group_import {
  uint32_t g0;                        /* the records land at local groups [g0, g0 + header.n) */
  uint32_t flags;                     /* JG_MOVE_DEVICE or 0                                  */
  int64_t shift_ms;                   /* added (wrapping) to election_time and heartbeat_time */
  const void* records;                /* header.n records                                     */
  jg_group_image_header header;       /* as the export wrote it                               */
} jg_group_import;
int jg_engine_export_groups(jg_engine* e, jg_group_export* x);
int jg_engine_import_groups(jg_engine* e, const jg_group_import* x);

/* ---- vacant slots: opening and closing partitions at runtime (ABI v13) ------------------------------
 * A slot is HOSTED (it holds a partition's Raft state) or VACANT (it hosts none).  A vacant slot has no
 * state that evolves: every command row addressed to it is ignored - JG_CMD_RESTART and JG_CMD_RECREATE
 * included - it emits no message, fsm or fault row and writes "nothing" into every outbox column, the
 * dense entry points, compaction and routed rounds leave it alone.  jg_read_state(JG_FIELD_FAULT) reads
 * JG_FAULT_VACANT, jg_engine_read_chains reads it as no rows and no commit key with that code, and
 * jg_drain_faults never reports it.  The vacant state is canonical: term 0, no vote, no leader, no
 * queue, Chain::new's genesis only (commit = head = 0, id_gen = 1), every progress head 0 in Probe,
 * heartbeat and election time 0 - only the own replica slot and the timeout RNG's draw count are kept,
 * so a slot closed and reopened never reuses a draw.  export_groups of a vacant slot is that record, and
 * importing it makes the destination slot vacant.
 *   - jg_engine_open_groups: every listed slot, which must be vacant, becomes what a JG_CMD_RECREATE row
 *     applied at now_ms makes of a slot (Raft::<Follower>::new on an empty data directory, the next
 *     timeout draw under the engine's seed, the slot's global id and its carried draw count); with
 *     self_slots the own replica slot is set per listed slot.  A partition whose sled tree exists is
 *     opened by jg_engine_load_chains over its range instead: the load overwrites a vacant slot as it
 *     overwrites any slot.
 *   - jg_engine_close_groups: every listed slot, which must be hosted, becomes vacant without emitting
 *     anything; rows it produced before stay in the drains.
 *   - both refuse with JG_EINVAL and write nothing for: an index out of range, a list that is not strictly
 *     ascending, opening a hosted slot or closing a vacant one, self_slots[i] >= R, queued commands, kept
 *     node steps.  Every entry is checked on the device before the pass that writes.
 *   - the set: groups == NULL is the range g0 .. g0 + n - 1; else n local indices, strictly ascending, in
 *     host memory or with JG_GROUPS_DEVICE in the engine's own device memory (a multi-device parent
 *     handle takes host lists: it splits them by shard, checks every shard, then writes).
 *   - jg_engine_list_groups: which = JG_LIST_VACANT or JG_LIST_HOSTED over local slots g0 .. g0 + n - 1;
 *     the first min(cap, total) matching indices, ascending, into `out` (host memory), *total = the number
 *     of matches (cap 0: the count only). */
enum { JG_GROUPS_DEVICE = 1u };       /* jg_group_set.flags: groups / self_slots are in the engine's device memory */
enum { JG_LIST_VACANT = 0u, JG_LIST_HOSTED = 1u };
typedef struct jg_group_set {
  uint32_t g0, n;                     /* groups == NULL: the range g0 .. g0 + n - 1                 */
  const uint32_t* groups;             /* [n] local indices, STRICTLY ascending                      */
  const uint8_t* self_slots;          /* open only: [n] own slot per listed slot, NULL: keep        */
  uint32_t flags, reserved;           /* JG_GROUPS_*                                                */
} jg_group_set;
int jg_engine_open_groups(jg_engine* e, uint64_t now_ms, const jg_group_set* s);
int jg_engine_close_groups(jg_engine* e, const jg_group_set* s);
int jg_engine_list_groups(jg_engine* e, uint32_t which, uint32_t g0, uint32_t n, uint32_t* out, size_t cap, size_t* total);

/* ---- the leadership feed and the census (ABI v14) ---------------------------------------------------
 * Which partitions changed leader, who leads them now, and how many of each kind there are - answered on
 * the device, so that a quiet engine costs a poll a few launches and 8 bytes over the bus instead of six
 * jg_read_state columns and a diff on the host.
 *
 * The LEADERSHIP VIEW of a slot is a function of columns jg_read_state exposes (role, term, leader id,
 * has-leader, fault, self slot) and nothing else:
 *   - a leader:                 leader_id = node_ids[self_slot], state = KNOWN | SELF (the leader-id column,
 *                               stale for a leader, is not consulted)
 *   - a follower that knows a leader (follower.rs:20): leader_id = that id, state = KNOWN
 *   - a candidate, a follower that knows none: leader_id = 0, no KNOWN
 *   - a vacant slot (fault 255): state = VACANT, fault = 255, every other field 0 but self_slot
 *   - a faulted slot (any other nonzero fault): as above from its frozen columns, FAULTED or-ed in
 *
 * jg_engine_watch_leaders compares the view of local slots g0 .. g0 + n - 1 with the engine's SHADOW - the
 * view it last reported per slot, device memory allocated at the first call (16 bytes per slot; an engine
 * that never watches pays nothing).  *total = the slots that differ in any field but group / self_slot;
 * `out` (host memory) receives the first min(cap, total) of them ascending, as their current view; cap 0:
 * the count only.  Exactly the slots whose rows were delivered become "seen": a small cap loses nothing
 * (the rest is pending at the next call), and a delivered slot is reported again only when its view
 * changes again.  JG_WATCH_PEEK delivers the same rows and advances nothing.  A watch starts as if every
 * slot had last been reported vacant: a fresh hosted engine reports every slot once (followers at term 0),
 * a JG_CFG_START_VACANT engine nothing until slots are opened.  Control-plane calls (open / close / load /
 * import) are seen through the diff alone.  ONE feed per engine - the handle has one owner (server.rs:103-
 * 165): two consumers of one engine would steal each other's changes.
 *
 * jg_engine_census counts what is over local slots g0 .. g0 + n - 1 in one reduction pass: integers,
 * exact whatever order the reduction runs in.
 *
 * Both calls READ: they settle JG_NODE_ASYNC steps, refuse with JG_EINVAL while kept node steps are
 * outstanding (as jg_engine_read_chains does; the kept steps stay viewable), and change nothing a step, a
 * drain or jg_read_state can observe.  JG_EINVAL too for a null `total` / `out` (census), a null `out`
 * with cap > 0, an unknown flag, a range out of bounds.  A multi-device parent handle answers in global
 * slot order with `cap` over the whole answer (every shard is sized first, so a shard behind the point
 * where cap ran out does not advance its shadow); its census is the shards' sum, max_term their maximum. */
enum { JG_LEAD_KNOWN = 1u, JG_LEAD_SELF = 2u, JG_LEAD_VACANT = 4u, JG_LEAD_FAULTED = 8u };  /* jg_leader_row.state */
enum { JG_WATCH_PEEK = 1u };          /* jg_engine_watch_leaders flags */
typedef struct jg_leader_row {        /* 24 bytes */
  uint32_t group;                     /* local slot (a sharded handle: index within the parent)     */
  uint32_t leader_id;                 /* NodeId of the leader this replica knows, 0: none           */
  uint64_t term;                      /* State.current_term                                         */
  uint8_t role;                       /* JG_ROLE_*                                                  */
  uint8_t state;                      /* JG_LEAD_*                                                  */
  uint8_t fault;                      /* JG_FAULT_* (255: vacant)                                   */
  uint8_t self_slot;
  uint32_t reserved;                  /* 0                                                          */
} jg_leader_row;
typedef struct jg_census {
  uint64_t hosted, vacant;
  uint64_t faulted_reference, faulted_engine;  /* fault 1..127, 128..254                            */
  uint64_t followers, candidates, leaders;     /* hosted and not faulted, by role                   */
  uint64_t leaderless;                /* hosted, not faulted, no leader known                       */
  uint64_t led_by[JG_MAX_REPLICAS];   /* ... known leader == node_ids[k]                            */
  uint64_t led_by_other;              /* ... known leader outside the membership                    */
  uint64_t max_term;                  /* over hosted slots, faulted included; 0 if none             */
  uint64_t uncommitted;               /* sum of head - commit over the healthy leaders, mod 2^64    */
} jg_census;
int jg_engine_watch_leaders(jg_engine* e, uint32_t flags, uint32_t g0, uint32_t n, jg_leader_row* out, size_t cap, size_t* total);
int jg_engine_census(jg_engine* e, uint32_t g0, uint32_t n, jg_census* out);

/* ---- the replication feed and census (ABI v15) ------------------------------------------------------
 * Which replicas of the partitions this engine leads are in sync, and which member is falling behind -
 * the data of Partition.isr (src/broker/state/partition.rs:15), which the reference reports to every
 * client (metadata.rs:93) and never maintains.  The facts live in the leader's ReplicationProgress
 * (progress.rs:42-60,124); here they are decided on the device from 16 bytes per slot instead of
 * 8R + 14 bytes of jg_read_state columns and a threshold and diff on the host.
 *
 * The REPLICATION VIEW is defined over columns jg_read_state exposes.  A slot LEADS for this feed if its
 * role is leader and its fault is 0 (a vacant, a faulted slot, a follower, a candidate do not); for a slot
 * that does not lead the view is all zero but group / self_slot.  For one that leads, with own slot s and
 * every member slot r < R:
 *   - lag_r = HEAD > MATCH_r ? HEAD - MATCH_r : 0 (saturating: a forged ack above the head counts as
 *     caught up, and so does a progress head between head and the run's top on a restarted leader)
 *   - the own slot is in sync by definition (MATCH_s is not consulted)
 *   - membership is HYSTERETIC against what was last reported: was_r = the shadow says this slot led and
 *     had bit r; in_r = was_r ? lag_r <= leave_lag : lag_r <= join_lag - a follower hovering at one
 *     threshold would otherwise produce a row every tick
 *   - isr: bit r = in_r; state = JG_ISR_LEADS | (popcount(isr) < R ? JG_ISR_UNDER : 0) |
 *     (popcount(isr) < R / 2 + 1 ? JG_ISR_BELOW_QUORUM : 0)
 *   - informational, NOT compared: replicate (the JG_FIELD_REPL_STATE mask), head, and worst_lag = the
 *     largest lag_r over r != s (0 at R = 1)
 *
 * jg_engine_watch_replicas compares the view of local slots g0 .. g0 + n - 1 with the engine's SHADOW -
 * the (isr, LEADS) it last reported per slot, device memory of its own allocated at the first call
 * (4 bytes per slot; independent of the leadership feed's shadow).  *total = the slots whose (isr, LEADS)
 * differs; `out` (host memory) receives the first min(cap, total) of them ascending, as their current
 * view; cap 0: the count only.  Exactly the slots whose rows were delivered become "seen": a small cap
 * loses nothing, JG_WATCH_PEEK delivers the same rows and advances nothing.  A zero-filled shadow means
 * "not leading, empty set": a fresh engine reports nothing until something leads; a NEW LEADER reports
 * {self}, and then each follower as its first acks arrive (join_lag applies to it; its members' progress
 * starts at 0, so a leader whose head is within join_lag of 0 reports them at once).  Open, close, load,
 * import and a loss of leadership are seen through the diff alone.  ONE feed per engine.
 *
 * jg_engine_replication_census is stateless: one threshold, no hysteresis, no shadow - a member of a led
 * slot is in sync iff its lag <= lag_limit (the own slot always).  Integers, exact whatever order the
 * reduction runs in.  out_of_sync[r] / max_lag[r] answer "which broker is slow".
 *
 * Both calls READ under the rules of the leadership feed: JG_NODE_ASYNC steps are settled first, JG_EINVAL
 * while kept node steps are outstanding, for a null `e` / `total` / `out` (census) / policy, a null `out`
 * with cap > 0, an unknown flag, a range out of bounds, join_lag > leave_lag.  A multi-device parent
 * handle answers in global slot order with `cap` over the whole answer (every shard is sized first by a
 * peek that delivers nothing; a shard behind the point where cap ran out keeps its shadow); its census
 * sums the counts and the lag sums and takes the maximum of the maxima. */
enum { JG_ISR_LEADS = 1u, JG_ISR_UNDER = 2u, JG_ISR_BELOW_QUORUM = 4u };  /* jg_isr_row.state */
typedef struct jg_isr_policy { uint64_t leave_lag, join_lag; } jg_isr_policy;   /* join_lag <= leave_lag */
typedef struct jg_isr_row {           /* 24 bytes: three 8-byte pieces */
  uint32_t group;                     /* local slot (a sharded handle: index within the parent)     */
  uint8_t isr;                        /* bit r: member r is in sync                                 */
  uint8_t replicate;                  /* bit r: progress of r is Replicate (JG_FIELD_REPL_STATE)    */
  uint8_t state;                      /* JG_ISR_*                                                   */
  uint8_t self_slot;
  uint64_t head;                      /* Chain.head of a slot that leads, else 0                    */
  uint64_t worst_lag;                 /* max lag over the members but the own slot                  */
} jg_isr_row;
typedef struct jg_repl_census {
  uint64_t leaders, fully_replicated, under_replicated, below_quorum;
  uint64_t out_of_sync[JG_MAX_REPLICAS];   /* led slots where member r has lag > lag_limit (own slot never) */
  uint64_t max_lag[JG_MAX_REPLICAS];       /* over the led slots, own slot 0                        */
  uint64_t sum_lag[JG_MAX_REPLICAS];       /* mod 2^64                                              */
  uint64_t max_uncommitted;                /* max of head - commit over the led slots               */
} jg_repl_census;
int jg_engine_watch_replicas(jg_engine* e, uint32_t flags, const jg_isr_policy* p, uint32_t g0, uint32_t n, jg_isr_row* out, size_t cap, size_t* total);
int jg_engine_replication_census(jg_engine* e, uint64_t lag_limit, uint32_t g0, uint32_t n, jg_repl_census* out);

/* ---- the replication feed under the time rule (ABI v19) ----------------------------------------------
 * replica.lag.time.max.ms: a member leaves the in-sync set once it has been BEHIND for longer than
 * max_behind_ms, not once it is some number of blocks behind - a block threshold has no right value (low, a
 * bursty producer evicts healthy followers; high, a dead follower of a slow partition is never noticed).
 *
 * jg_engine_watch_replicas_timed is jg_engine_watch_replicas under another membership rule: the rows, the
 * `state` bits, replicate / head / worst_lag, the ascending order, cap, total and JG_WATCH_PEEK are the
 * same, and it shares the SHADOW - the (isr, LEADS) last delivered - with it: ONE feed, so the two calls
 * and jg_engine_poll may be mixed.  New is one piece of feed memory, the CLOCKS, allocated zero-filled at
 * the first timed call: stamp[r][g], 8 bytes per member and slot; 0 = "not behind at the last sample", any
 * other value = now_ms + 1 of the first sample that saw the member behind.
 *
 * Per slot g of the range, lag_r as above (saturating) and was_r from the shadow:
 *   - the slot does not lead (role != leader, or fault != 0, or vacant): the view is 0 and every clock of
 *     the slot becomes 0
 *   - it leads, own slot s: bit s is set, its clock is ignored
 *   - it leads, member r != s:
 *       c'        = lag_r <= caught_lag ? 0 : (stamp ? stamp : now_ms + 1)
 *       behind_ms = c' ? (now_ms + 1 > c' ? now_ms + 1 - c' : 0) : 0     (saturating: a clock that steps
 *                   back evicts nobody)
 *       in_r      = was_r ? behind_ms <= max_behind_ms : lag_r <= join_lag
 *   - isr, state and "differs from the shadow" are then as in the lag feed
 * A call WITHOUT JG_WATCH_PEEK stores stamp := c' (or 0) for EVERY slot of g0 .. g0 + n - 1, whether or not
 * the slot's row fits cap and whether or not it differs: time passes for a row that was not delivered.
 * Advancing twice at one now_ms on unchanged state is idempotent.  The shadow advances for exactly the
 * delivered slots, as in the lag feed.  A call WITH JG_WATCH_PEEK computes with c' and writes neither clocks
 * nor shadow.
 *
 * What follows from that:
 *   - the clock is SAMPLED: its resolution is the poll period, and a member is never seen behind for
 *     longer than the samples show
 *   - a follower already down at the first timed call leaves max_behind_ms after that call
 *   - a slot that stops leading and leads again between two samples keeps its clocks, as it keeps its shadow
 *   - under continuous appends a follower that is always a few blocks behind is "behind" at every sample:
 *     caught_lag has to be at least what is in flight per sample
 *   - max_behind_ms = UINT64_MAX: nobody ever leaves; 0: a member leaves at the first sample after the
 *     one that saw it fall behind, provided the clock has moved
 *
 * It READS under the rules of jg_engine_watch_replicas and is refused with JG_EINVAL - nothing written, no
 * clock and no shadow advanced - wherever that call is (a null `e` / `total`, a null `out` with cap > 0, an
 * unknown flag, a range out of bounds, kept node steps outstanding), for a null clock, now_ms ==
 * UINT64_MAX and join_lag > caught_lag.  n = 0 is JG_OK with total 0.  A multi-device parent handle answers
 * in global slot order with `cap` over the whole answer; without JG_WATCH_PEEK the clocks of EVERY shard
 * advance, those behind the point where cap ran out too. */
typedef struct jg_isr_clock {
  uint64_t now_ms;         /* the caller's clock at this sample; UINT64_MAX is refused            */
  uint64_t max_behind_ms;  /* replica.lag.time.max.ms; UINT64_MAX: never leaves                   */
  uint64_t caught_lag;     /* a member with lag <= this is "caught up" at this sample (0 = strict) */
  uint64_t join_lag;       /* a member outside the set joins at lag <= this; join_lag <= caught_lag */
} jg_isr_clock;
int jg_engine_watch_replicas_timed(jg_engine* e, uint32_t flags, const jg_isr_clock* c, uint32_t g0, uint32_t n, jg_isr_row* out, size_t cap, size_t* total);

/* ---- point queries: the state of a list of partitions (ABI v16) --------------------------------------
 * "What is the state of exactly these partitions" - Metadata for some topics, the high watermark of the
 * 500 partitions of a Fetch, the 2 000 a controller just moved - in one call: the batched form of
 * RaftHandle's introspection (is_leader, get_term, ..., src/raft/mod.rs:437-468).  jg_read_state answers
 * it per field over a range (one copy per column, decoded on the host) or per slot and field (two or more
 * synchronous copies each); here one device pass gathers every field of every listed slot into one row.
 *   - ANSWER ORDER: out[i] describes s->groups[i], in the order asked.  Unlike open and close the list need
 *     NOT be ascending and MAY repeat an index: a request names partitions in its own order.
 *   - groups == NULL is the range g0 .. g0 + n - 1: every jg_read_state field of a range in one pass.
 *     self_slots is ignored.
 *   - each field named after a JG_FIELD_* holds exactly the value jg_read_state returns for that field and
 *     slot: a leader's commit decoded from the packed word, id_gen implicit while the chain is in FAST form,
 *     leader_id 0 unless a follower that knows one, heartbeat_time 0 unless leader, the vote masks 0 unless
 *     candidate, and so on.
 *   - `state` and `known_leader` are the LEADERSHIP VIEW of jg_engine_watch_leaders (jg_leader_row.state /
 *     .leader_id).  A vacant slot is JG_LEAD_VACANT with fault 255 and the canonical vacant columns.
 *   - JG_LOOKUP_PROGRESS (needs match != NULL): match[i * R + r] = JG_FIELD_MATCH of replica r of entry i,
 *     0 for a slot that is not a leader.  Without the flag `match` is not touched.
 *   - it READS: it settles JG_NODE_ASYNC steps, refuses with JG_EINVAL while kept node steps are outstanding
 *     (the kept steps stay viewable), does not see queued, unstepped commands, and changes nothing a step, a
 *     drain, a feed or jg_read_state can observe.
 *   - JG_EINVAL with `out` and `match` untouched for: a null `s`, a null `out` with n > 0, an unknown flag, an
 *     index or a range out of bounds, JG_LOOKUP_PROGRESS without `match`, JG_GROUPS_DEVICE on a multi-device
 *     parent handle.  A host list is checked on the host before anything is queued; a device list
 *     (JG_GROUPS_DEVICE: the engine's own device memory) is checked on the device before any byte is copied
 *     to the caller.  n = 0 is JG_OK.
 *   - a multi-device parent handle takes a host list (or a range), lets every shard look up its entries and
 *     answers in the order asked; `group` is the index within the parent. */
enum { JG_LOOKUP_PROGRESS = 2u };     /* jg_group_set.flags for a lookup (bit 0 stays JG_GROUPS_DEVICE) */
typedef struct jg_group_state {       /* 80 bytes: five 16-byte pieces */
  uint32_t group;                     /* the index as asked (a sharded handle: index within the parent) */
  uint32_t known_leader;              /* the leadership view's leader_id (jg_leader_row.leader_id)      */
  uint64_t term, head, commit, id_gen;            /* JG_FIELD_TERM / HEAD / COMMIT / ID_GEN             */
  uint64_t election_time, heartbeat_time;         /* JG_FIELD_ELECTION_TIME / HEARTBEAT_TIME            */
  uint32_t voted_for, leader_id;                  /* JG_FIELD_VOTED_FOR / LEADER_ID                     */
  uint32_t election_timeout, queued_reqs;         /* JG_FIELD_ELECTION_TIMEOUT / QUEUED_REQS            */
  uint8_t role, state, fault, self_slot;          /* JG_FIELD_ROLE, JG_LEAD_* bits, FAULT, SELF_SLOT    */
  uint8_t repl_state, vote_seen, vote_granted;    /* JG_FIELD_REPL_STATE / VOTE_SEEN / VOTE_GRANTED     */
  uint8_t has;                                    /* bit 0 JG_FIELD_HAS_VOTED, bit 1 JG_FIELD_HAS_LEADER */
} jg_group_state;
int jg_engine_lookup_groups(jg_engine* e, const jg_group_set* s, jg_group_state* out, uint64_t* match /* [n][R] or NULL */);

/* ---- the commit feed: what dense steps committed and appended (ABI v17) -------------------------------
 * "Which partitions' high watermark advanced since I last looked, and from where to where?  Which got new
 * blocks?" - the data of fsm::Driver (src/fsm.rs:20-93), of a Fetch long-poll, of a follower's store
 * catching up.  The dense entry points (jg_step_dense_acks*, jg_step_dense_leader / _follower,
 * jg_dense_cluster_rounds, the dense halves of jg_dense_cluster_round_routed) queue no FSM rows: their
 * instructions are the per-group head / commit deltas.  Instead of two whole-range jg_read_state columns
 * (16 bytes per slot over the bus) and a diff on the host per poll, the diff is made on the device.
 *
 * The COMMIT VIEW of a slot is (commit, head) exactly as jg_read_state returns JG_FIELD_COMMIT and
 * JG_FIELD_HEAD: a leader's commit decoded from the packed word (the escape to the wide column and a base
 * that is the run's top included); a vacant slot's view is (0, 0), a faulted slot's its frozen columns.
 *
 * The SHADOW is (commit_from, head_from) as last delivered: 16 bytes per slot, device memory of its own
 * allocated zero-filled at the first call, independent of the other two feeds' shadows.  Zero means
 * "genesis only": a fresh engine and a JG_CFG_START_VACANT engine report nothing until something is
 * appended or committed.
 *
 * jg_engine_watch_commits compares the view of local slots g0 .. g0 + n - 1 with the shadow.  A slot
 * DIFFERS iff commit != commit_from || head != head_from; with JG_WATCH_COMMITS_ONLY iff commit !=
 * commit_from (a high-watermark consumer, which should not get a row for every append of a follower).
 * *total = the slots that differ; `out` (host memory) receives the first min(cap, total) of them
 * ascending; cap 0: the count only.  Exactly the delivered slots have BOTH shadow words advanced to the
 * row's commit / head (under JG_WATCH_COMMITS_ONLY too): a small cap loses nothing, JG_WATCH_PEEK
 * delivers the same rows and advances nothing.  ONE feed per engine, as for the other feeds.
 *
 * state: JG_CMT_COMMITTED commit > commit_from; JG_CMT_APPENDED head > head_from; JG_CMT_REWOUND either
 * value went DOWN (a restart - head = commit -, a recreate, a close, a load, an import: the consumer
 * resynchronises its store instead of applying a range); JG_CMT_LEADS role leader and fault 0;
 * JG_CMT_VACANT fault 255; JG_CMT_FAULTED any other nonzero fault.  role / fault / self_slot are
 * JG_FIELD_ROLE / FAULT / SELF_SLOT now; term is JG_FIELD_TERM now, informational and NOT compared.
 *
 * EXPANDING a row is the caller's convention, as the dense entry points document it: a leader - Apply for
 * keys (commit_from, commit], Notify for ids (head_from, head]; a follower - Apply for keys
 * [commit_from, commit) (JG_FSM_APPLY_LEADER / JG_FSM_APPLY_FOLLOWER {a = commit_from, b = commit}).
 * Consecutive ranges concatenate exactly where the role did not change between two deliveries; a consumer
 * that must know about a role change polls the leadership feed (jg_engine_watch_leaders) first.
 *
 * backlog, where not NULL, is filled from the counting pass: the state BEFORE this call's delivery, over
 * EVERY slot of the range that differs (under the call's flags), delivered or not.  changed == *total.
 * Integers, exact whatever order the reduction runs in.
 *
 * The call READS under the rules of jg_engine_watch_replicas: JG_NODE_ASYNC steps are settled first; it
 * changes nothing a step, a drain, a read or the other feeds can observe; JG_EINVAL - with `out`, `total`,
 * `backlog` and the shadow untouched - while kept node steps are outstanding, for a null `e` / `total`, a
 * null `out` with cap > 0, an unknown flag, a range out of bounds.  A multi-device parent handle sizes
 * every shard by a peek that delivers nothing (the backlog is the shards' sum from that pass), then each
 * shard delivers into what is left of `cap`, in global slot order; a shard behind the point where cap ran
 * out keeps its shadow.  Reading a node of a jg_dense_cluster between rounds is allowed. */
enum { JG_CMT_COMMITTED = 1u, JG_CMT_APPENDED = 2u, JG_CMT_REWOUND = 4u,
       JG_CMT_LEADS = 8u, JG_CMT_VACANT = 16u, JG_CMT_FAULTED = 32u };   /* jg_commit_row.state */
enum { JG_WATCH_COMMITS_ONLY = 2u };   /* flags of jg_engine_watch_commits (bit 0 stays JG_WATCH_PEEK) */
typedef struct jg_commit_row {         /* 48 bytes: three 16-byte pieces */
  uint32_t group;                      /* local slot (a sharded handle: index within the parent) */
  uint8_t role, state, fault, self_slot;
  uint64_t term;                       /* JG_FIELD_TERM now - informational, NOT compared */
  uint64_t commit_from, commit;        /* as last delivered / JG_FIELD_COMMIT now */
  uint64_t head_from, head;            /* as last delivered / JG_FIELD_HEAD now   */
} jg_commit_row;
typedef struct jg_commit_backlog {     /* over ALL slots of the range that differ, delivered or not */
  uint64_t changed, committed, appended, rewound;
  uint64_t pending_commits;            /* sum of commit - commit_from where commit > commit_from, mod 2^64 */
  uint64_t pending_appends;            /* sum of head - head_from where head > head_from, mod 2^64 */
} jg_commit_backlog;
int jg_engine_watch_commits(jg_engine* e, uint32_t flags, uint32_t g0, uint32_t n, jg_commit_row* out, size_t cap, size_t* total,
                            jg_commit_backlog* backlog /* may be NULL */);

/* ---- the completion feed: fsm::Driver's notifications on the device (ABI v22) --------------------------
 * "Which of the produce requests I am holding can be answered now, and how?" - the reference keeps
 * notifications: HashMap<BlockId, (Address, ClientRequestId)> (src/raft/fsm.rs:35): Instruction::Notify
 * (leader.rs:184-188) inserts, every Instruction::Apply looks its block id up and sends the
 * ClientResponse (fsm.rs:65-76).  On the dense path a caller would expand every commit row into single
 * block keys and probe a map once per key.  Here the WAITERS (partition, block id, token) live in device
 * memory and one call per tick answers which tokens are done, and why - applied, lost (not leader any
 * more: retry elsewhere), expired (timed out): a produce purgatory.
 *
 * jg_engine_await_open (re)sizes the TABLE to `capacity` waiters (two buffers of 48 bytes a waiter, a
 * verdict byte each, the scan's scratch); 0 frees it.  JG_EINVAL while waiters are outstanding.
 *
 * jg_engine_await_blocks registers n waiters behind the table's end, ALL OR NOTHING: JG_EINVAL - with
 * nothing registered - for a null argument, a group >= G, nonzero flags or reserved, block_id == 0 (the
 * reference skips block 0, fsm.rs:61), no open table; JG_ECAPACITY when outstanding + n > capacity; n == 0
 * is JG_OK.  token is opaque and returned as given.  term == 0 selects the reference's rule, term != 0
 * guards the waiter by leadership.  deadline_ms == 0: the waiter never expires.
 *
 * A waiter's VERDICT is decided at a watch, from its slot's state as jg_read_state would return it then -
 * role, fault, JG_FIELD_TERM, JG_FIELD_COMMIT (decoded exactly as the commit feed and the point queries
 * do), JG_FIELD_HEAD.  The first rule that matches wins:
 *   0. (ABI v24) withdrawn by jg_engine_await_cancel -> JG_DONE_CANCELLED, whatever the slot looks like
 *   1. fault 255 -> JG_DONE_LOST | JG_DONE_VACANT; any other nonzero fault -> JG_DONE_LOST | JG_DONE_FAULTED
 *   2. term != 0 and (role is not leader or JG_FIELD_TERM != term) -> JG_DONE_LOST.  Deliberately BEFORE
 *      the applied test: a block that committed under a later leadership cannot be told from a different
 *      block with the same id.  The client retries: at-least-once, as Kafka gives
 *   3. applied -> JG_DONE_APPLIED: the slot leads (role leader, fault 0) and block_id <= commit, or it does
 *      not lead and block_id < commit - the two key conventions of the commit feed, leader (commit_from,
 *      commit], follower [commit_from, commit), applied from genesis
 *   4. deadline_ms != 0 and now_ms >= deadline_ms -> JG_DONE_EXPIRED
 *   5. otherwise the waiter keeps waiting
 *
 * TWO DEPARTURES from the reference.  Every registered waiter is answered exactly once: registering a key
 * twice answers both, where the reference's map would forget the first (its leader never does this:
 * Chain::append draws a fresh id each time).  And applied is a WATERMARK, not an event: an id already
 * under the watermark at registration completes at the next watch, where the reference's Apply for it
 * has passed and it would never answer (Notify always precedes the commit that applies it, so the
 * reference's own callers cannot tell the difference).
 *
 * jg_engine_watch_completions: the table keeps REGISTRATION ORDER.  *total = the done waiters; `out`
 * (host memory) receives the first min(cap, total) of them in that order; cap 0: counts only.  The watch
 * removes exactly the delivered waiters, the survivors keep their relative order; a done waiter beyond
 * cap is a survivor.  JG_WATCH_PEEK delivers the same rows and removes nothing.  A row: group, the
 * verdict in `state`, role / fault / self_slot, JG_FIELD_TERM / COMMIT / HEAD now, token and block_id as
 * registered.  stats, where not NULL: waiting / done / applied / lost / expired describe the state BEFORE
 * this call's delivery over EVERY waiter (done == *total), left = the waiters outstanding after the call.
 * Integers, exact whatever order the reduction runs in.
 *
 * Both calls READ under the rules of the other feeds: JG_NODE_ASYNC steps are settled first; nothing a
 * step, a drain, a read or another feed can observe changes; JG_EINVAL - with nothing written - while
 * kept node steps are outstanding, for an unknown flag, for now_ms == UINT64_MAX, a null `e` / `total`, a
 * null `out` with cap > 0.  A watch on an engine without a table is JG_OK with total 0.  A multi-device
 * parent handle buckets the rows by owner shard, stably; each shard has a table of its own and `capacity`
 * is per shard; a watch sizes every shard by a peek (the stats are the shards' sums), then each shard
 * delivers into what is left of `cap`, in shard order, `group` the parent's index; a shard behind the
 * point where cap ran out keeps its waiters. */
enum { JG_DONE_APPLIED = 1u, JG_DONE_LOST = 2u, JG_DONE_EXPIRED = 4u,
       JG_DONE_VACANT = 8u, JG_DONE_FAULTED = 16u,
       JG_DONE_CANCELLED = 32u };                      /* jg_done_row.state (CANCELLED: ABI v24) */
/* jg_await_row.flags as the TABLE keeps it: the waiter was withdrawn by jg_engine_await_cancel.  The table's
 * own bit - never accepted from a caller: registration refuses any nonzero flags. */
enum { JG_AWAIT_WITHDRAWN = 1u };
typedef struct jg_await_row {          /* 48 bytes: three 16-byte pieces */
  uint32_t group;                      /* local slot (a sharded handle: index within the parent) */
  uint32_t flags;                      /* must be 0 (the table keeps JG_AWAIT_WITHDRAWN here) */
  uint64_t token;                      /* opaque: returned as given (jg_engine_await_cancel matches it under a mask) */
  uint64_t block_id;                   /* != 0 */
  uint64_t term;                       /* 0: the reference's rule; else the leadership the waiter is guarded by */
  uint64_t deadline_ms;                /* 0: never expires */
  uint64_t reserved;                   /* must be 0 */
} jg_await_row;
typedef struct jg_done_row {           /* 48 bytes: three 16-byte pieces */
  uint32_t group;                      /* local slot (a sharded handle: index within the parent) */
  uint8_t state, role, fault, self_slot;   /* JG_DONE_* bits; JG_FIELD_ROLE / FAULT / SELF_SLOT now */
  uint64_t token;
  uint64_t block_id, term_now;         /* as registered / JG_FIELD_TERM now */
  uint64_t commit_now, head_now;       /* JG_FIELD_COMMIT / JG_FIELD_HEAD now */
} jg_done_row;
typedef struct jg_await_stats {
  uint64_t waiting, done, applied, lost, expired;   /* before this call's delivery, over every waiter */
  uint64_t left;                                    /* outstanding after the call */
} jg_await_stats;                      /* the verdicts are exclusive: cancelled = done - applied - lost - expired */
int jg_engine_await_open(jg_engine* e, size_t capacity);
int jg_engine_await_blocks(jg_engine* e, const jg_await_row* rows, size_t n);
int jg_engine_watch_completions(jg_engine* e, uint32_t flags, uint64_t now_ms, jg_done_row* out, size_t cap, size_t* total,
                                jg_await_stats* stats /* may be NULL */);

/* ---- withdrawing waiters: a closed connection leaves the purgatory (ABI v24) ---------------------------
 * A waiter otherwise leaves the table only applied, lost or expired: a client that hangs up while its
 * request waits on a healthy leader, unguarded and without a deadline, would sit there for ever (the
 * reference's notifications map has the same leak: an entry goes only at the Apply that answers it).
 *
 * jg_engine_await_cancel MARKS, in place, every outstanding waiter whose (token & mask) is one of the n_keys
 * keys: mask = ~0 withdraws exact tokens; a caller that keeps a connection id in the token's high 32 bits
 * withdraws connections with mask = 0xFFFFFFFF00000000 and the ids << 32 as keys; mask = 0 with the single
 * key 0 withdraws everything (shutdown, or before a resize).  The keys are copied at entry, sorted, and
 * duplicates removed: any order will do.  *marked = the waiters NEWLY marked by this call (one that was
 * marked already is not counted again).
 *
 * RULE 0 of the verdict, ahead of rule 1: a marked waiter is done with state == JG_DONE_CANCELLED - that
 * bit alone, whatever its slot looks like (vacant, faulted, deposed, applied, past its deadline).  Everything
 * else is the feed as it stands: the waiter is delivered as a jg_done_row in registration order, subject to
 * cap and JG_WATCH_PEEK, with the slot's fields as they are at that watch, exactly once; the mark is stored
 * in the waiter, so it survives a compaction and a watch whose cap ran out before it.  A cancel removes
 * nothing: a cancelled waiter counts as outstanding until a watch delivers it.  Waiters registered after
 * the call are not affected by it.  In jg_await_stats a cancelled waiter counts in `done` and in none of
 * applied / lost / expired.
 *
 * n_keys == 0: JG_OK, 0 marked.  No open table: JG_OK, 0 marked (as a watch).  JG_EINVAL - nothing written,
 * nothing marked - for a null `e` or `marked`, null `keys` with n_keys > 0, n_keys > JG_AWAIT_CANCEL_MAX, a
 * key with a bit outside `mask` (it could never match: a caller's bug), and while kept node steps are
 * outstanding; JG_NODE_ASYNC steps are settled first.  A multi-device parent sends the same keys to every
 * shard, *marked is the sum.  Reads nothing but the table and writes nothing but the marks: no step, drain,
 * read or other feed can observe it. */
#define JG_AWAIT_CANCEL_MAX 65536u
int jg_engine_await_cancel(jg_engine* e, const uint64_t* keys, size_t n_keys, uint64_t mask, size_t* marked);

/* ---- one poll per tick: the three feeds and the two censuses in one call (ABI v18) --------------------
 * An event loop that consumes several feeds asks them of the same slots once per tick.  Asked separately
 * every call is a round trip of its own: a settle, a count pass, a scan, a write pass, a synchronisation
 * and a blocking row copy.  jg_engine_poll answers all the parts `want` names with ONE settle, ONE device
 * pass over the slots (the flag word and the packed progress word read once: 88 bytes per slot instead
 * of 104), one scan launch and ONE synchronisation.  It defines no value of its own:
 *
 * CONTRACT.  Let S be the separate calls that `want` names - jg_engine_watch_leaders (JG_POLL_LEADERS:
 * leader_flags, leaders, leaders_cap, leaders_total), jg_engine_watch_replicas (JG_POLL_REPLICAS with
 * clock == NULL: replica_flags, policy, replicas, replicas_cap, replicas_total) or, since v20,
 * jg_engine_watch_replicas_timed (JG_POLL_REPLICAS with clock != NULL: replica_flags, clock, replicas,
 * replicas_cap, replicas_total; policy is then not read), jg_engine_watch_commits
 * (JG_POLL_COMMITS: commit_flags, commits, commits_cap, commits_total, backlog - may be NULL),
 * jg_engine_census (JG_POLL_CENSUS: census), jg_engine_replication_census (JG_POLL_REPL_CENSUS:
 * census_lag_limit, repl_census) - each over local slots g0 .. g0 + n - 1.  The poll leaves exactly what
 * S leaves when each is called on the same engine state: every output byte, every total, the backlog,
 * the three shadows and the replication feed's clocks (the stamps and their mask).  Under the time rule
 * and without JG_WATCH_PEEK in replica_flags the clocks of EVERY slot of the range advance to
 * clock->now_ms, delivered or not and whatever replicas_cap is, 0 included; with JG_WATCH_PEEK neither
 * clocks nor shadow are written.  *clock is copied at entry.  JG_POLL_REPL_CENSUS stays the lag gauge of
 * census_lag_limit whichever rule the feed runs under.  The feeds do not observe each other, so no order
 * among the parts is defined.
 * A part NOT named is not computed: its shadow is neither allocated nor advanced and its fields of
 * jg_poll are neither read nor written (clock is not dereferenced unless JG_POLL_REPLICAS is wanted).
 * The lag poll, the timed poll, jg_engine_watch_replicas and jg_engine_watch_replicas_timed share one
 * shadow and one set of clocks; the poll and the separate calls may be mixed freely on one engine.
 *
 * ALL OR NOTHING.  Every argument of every wanted part is checked before anything is queued, by the
 * separate calls' own rules: JG_EINVAL - no shadow and no clock advanced, no byte of any output or total
 * written - for a null `e` / `p`, want == 0 or an unknown bit, an unknown flag in a wanted feed's flag
 * word, join_lag > leave_lag in the policy of a wanted replicas part without a clock, now_ms ==
 * UINT64_MAX or join_lag > caught_lag in the clock of a wanted replicas part (the policy is then not
 * looked at: join_lag > leave_lag in it is no error), a null row array with a nonzero cap, a null census pointer of a wanted census, a range out
 * of bounds, kept node steps outstanding.  n == 0 is JG_OK with totals 0 and zeroed censuses and backlog.
 *
 * It READS: JG_NODE_ASYNC steps are settled once; nothing a step, a drain, jg_read_state or a separate
 * feed call can observe changes, the shadows as stated above excepted.  A multi-device parent handle
 * sizes every shard by one fused peek that delivers nothing (the backlog and the censuses are the shards'
 * sums or maxima from that pass), then each shard delivers into what is left of EACH feed's own cap, in
 * global slot order; a shard behind the point where a feed's cap ran out keeps that feed's shadow.
 * Under the time rule the sizing pass is no peek of the replicas part: it delivers nothing and, unless the
 * caller peeks, advances that shard's clocks; the delivering pass advances them again at the same now_ms,
 * which is idempotent.  A shard behind the point where the replicas' cap ran out keeps its shadow, and its
 * clocks have advanced. */
enum { JG_POLL_LEADERS = 1u, JG_POLL_REPLICAS = 2u, JG_POLL_COMMITS = 4u,
       JG_POLL_CENSUS = 8u, JG_POLL_REPL_CENSUS = 16u };   /* jg_poll.want */
typedef struct jg_poll {
  uint32_t want;                       /* JG_POLL_*; 0 is JG_EINVAL                              */
  uint32_t g0, n;                      /* local slots g0 .. g0 + n - 1, for every part           */
  uint32_t leader_flags;               /* JG_WATCH_PEEK                                          */
  uint32_t replica_flags;              /* JG_WATCH_PEEK                                          */
  uint32_t commit_flags;               /* JG_WATCH_PEEK | JG_WATCH_COMMITS_ONLY                  */
  jg_isr_policy policy;                /* JG_POLL_REPLICAS                                       */
  uint64_t census_lag_limit;           /* JG_POLL_REPL_CENSUS                                    */
  jg_leader_row* leaders;              /* out: host memory, [leaders_cap]                        */
  size_t leaders_cap, leaders_total;   /* in, out                                                */
  jg_isr_row* replicas;
  size_t replicas_cap, replicas_total;
  jg_commit_row* commits;
  size_t commits_cap, commits_total;
  jg_commit_backlog* backlog;          /* out, may be NULL                                       */
  jg_census* census;                   /* out: JG_POLL_CENSUS                                    */
  jg_repl_census* repl_census;         /* out: JG_POLL_REPL_CENSUS                               */
  const jg_isr_clock* clock;           /* JG_POLL_REPLICAS: NULL = the lag rule (policy); else the time rule, policy is not read */
} jg_poll;
int jg_engine_poll(jg_engine* e, jg_poll* p);

/* ---- shards of a multi-device engine ------------------------------------------------------------
 * Everything that takes HOST memory works on the parent handle exactly as on a single-device
 * engine: jg_submit buckets the rows by owner (stable: a group's rows keep their order), jg_step
 * steps every shard (one host thread and one HIP stream per shard), the drains merge the shards'
 * rows back into the single-engine order (per step: groups ascending; steps in order),
 * jg_read_state / jg_get_counters / jg_drain_faults / jg_sync / jg_set_self_slots /
 * jg_step_dense_acks (host [R][G] block) split or concatenate per shard.  Results are
 * bit-identical to one engine over the same G groups (tests/test_multi_device.py).
 * Everything that takes DEVICE pointers is per device by nature: the caller addresses a shard's
 * own engine handle (jg_get_shard; an ordinary single-device engine over groups
 * [group_lo, group_lo + n_groups), local group index = global - group_lo) for
 * jg_step_dense_leader / _follower, jg_step_device_rows, jg_device_*, jg_synth_fill_acks_device,
 * jg_calibrate_stream; jg_step_dense_acks_shards launches the ack tick on every shard at once.
 * Shard handles are owned by the parent: never destroy them, and do not drain them directly. */
typedef struct jg_shard_info {
  jg_engine* engine;  /* the shard's own single-device engine                                  */
  int32_t device_id;
  uint32_t group_lo;  /* first group (index within the parent) this shard owns                 */
  uint32_t n_groups;
  uint32_t reserved;
} jg_shard_info;
uint32_t jg_shard_count(const jg_engine* e); /* 1 for a single-device engine (which is its own shard) */
int jg_get_shard(jg_engine* e, uint32_t shard, jg_shard_info* out);

/* Per-group own replica slot (default: all 0).  Only legal before the first step. */
int jg_set_self_slots(jg_engine* e, const uint8_t* slots /* [G] host */);

/* Queue a batch of commands (host memory, borrowed for the call).  Rows may be in
 * any group order; rows of the same group are applied in row order, after rows
 * queued by earlier jg_submit calls. */
int jg_submit(jg_engine* e, const jg_cmd_batch* batch);

/* Zero-copy jg_submit for a caller that produces rows itself (a transport's receive task decoding
 * straight into the engine's pinned columns, src/raft/tcp.rs:139-170 -> server.rs:126-137): room for n
 * more rows and n_blocks side-array entries at the tail of the pending batch; the caller fills kind,
 * group, id and whichever optional columns it needs in place (an AppendEntries row's id indexes THIS
 * reservation's side-array entries) and commits how many it wrote, and which optional columns
 * (JG_COL_*): a column not named is all zeros for these rows and costs nothing - jg_step_node does not
 * even upload a column that no submit of the step provided.  jg_submit_commit checks what jg_submit
 * checks.  The pointers are good until the next jg_submit* or step call.  Single-device engines (or a
 * shard's own handle). */
typedef struct jg_cmd_cols {
  uint8_t* kind;
  uint32_t* group;
  uint32_t* from;
  uint64_t* term;
  uint64_t* id;
  uint64_t* aux;
  uint8_t* flag;
  uint64_t* blk_id;
  uint64_t* blk_next;
} jg_cmd_cols;
enum { JG_COL_FROM = 1u, JG_COL_TERM = 2u, JG_COL_AUX = 4u, JG_COL_FLAG = 8u,
       /* no validation pass over the rows on the host (it costs 2.5 ms per 9 M rows): jg_step_node's classification
        * checks group and kind on the device - a row out of range is not applied and the next synchronising call
        * returns JG_EINVAL.  Only jg_step_node takes such a batch (jg_step refuses it). */
       JG_COL_UNCHECKED = 16u,
       /* these rows are the whole batch of the next jg_step_node (nothing was committed before them since the last
        * step, nothing follows): their upload starts NOW, on a copy stream of its own - while the previous step's
        * kernels run and its outputs travel the other way - instead of at the head of the step.  A batch that turns
        * out not to be the step's whole input is simply uploaded again by the step. */
       JG_COL_UPLOAD_NOW = 32u,
       /* the kind column of these rows holds `kind | sender << 4 | flag << 7`: sender = the member slot (index into
        * jg_config.node_ids, 3 bits) of Message.from for the kinds that carry one (VoteRequest ... HeartbeatResponse;
        * a slot >= n_replicas reads as NodeId 0, the other kinds read 0 whatever the bits), flag as the flag column -
        * neither a `from` nor a `flag` column exists for the step (naming JG_COL_FROM / JG_COL_FLAG with it is an
        * error): an AppendResponse row is 13 bytes on the bus, not 18.  Every commit of a step must agree on it, it
        * needs JG_COL_UNCHECKED (the device decodes and checks the byte), and jg_submit cannot add rows to such a step. */
       JG_COL_PACKED_KIND = 64u,
       /* the id column of these rows holds 32-bit values: the caller writes n uint32_t at (uint32_t*)cols.id (block ids,
        * commit indices, request tokens, side-array indices - zero-extended on the device): 4 bytes per row on the bus
        * instead of 8.  Only as the step's ONE commit (no rows before it, none after it, no jg_submit in the step); needs
        * JG_COL_UNCHECKED. */
       JG_COL_ID32 = 128u };
int jg_submit_reserve(jg_engine* e, size_t n, size_t n_blocks, jg_cmd_cols* cols);
int jg_submit_commit(jg_engine* e, size_t n, size_t n_blocks, uint32_t optional_columns);

/* Apply everything queued since the last step: for each group, `apply(cmd)` in
 * stream order (src/raft/mod.rs:471-479).  `now_ms` is the logical clock that
 * replaces Instant::now() (mod.rs:352-357, follower.rs:110-113, leader.rs:78-84).
 * Outputs are appended to the message / fsm queues.  Asynchronous on the
 * engine's stream; drains and reads synchronise. */
int jg_step(jg_engine* e, uint64_t now_ms);

/* The same step for a batch that already lives in device memory: every pointer of
 * `dev_batch` is a device pointer (all seven columns required; the block side
 * arrays only if AppendEntries rows are present) and the rows MUST be sorted by
 * group, rows of one group in stream order — the form k_apply_rows consumes, so no
 * host pass is needed.  Unsorted rows or an out-of-range group are reported as
 * JG_EINVAL by the next synchronising call. */
int jg_step_device_rows(jg_engine* e, const jg_cmd_batch* dev_batch, uint64_t now_ms);

/* Dense steady-state leader tick (the HBM-roofline path).
 * `acks` is an [R][G] column-major array (replica-major: acks[r*G+g]):
 *   r != self_slot[g]: head of an AppendResponse{node_id: node_ids[r], head} or JG_NO_ACK;
 *   r == self_slot[g]: number of ClientRequests to append this tick, < JG_MAX_DENSE_APPENDS
                        (a larger value, JG_NO_ACK included, raises JG_FAULT_ENGINE_DENSE_APPENDS
                        on that group and applies nothing of its tick).
 * Per group, in this order: the appends (leader.rs:177-197, each with its
 * self-ack), then the acks in ascending slot order (leader.rs:211-219 ->
 * progress.rs:42-60 -> leader.rs:87-99).  Equivalent to submitting those
 * commands through jg_submit/jg_step, except that the FSM instructions are not
 * queued: they are the per-group head / commit deltas (Notify for ids
 * (head_before, head_after], Apply for keys (commit_before, commit_after]), which
 * the caller reads back with jg_read_state.  Non-leader groups ignore acks exactly as the
 * reference does (follower.rs:62, candidate.rs:194); asking one to append is a
 * precondition violation of the dense path (client proxying needs the message
 * queue of jg_step) and raises JG_FAULT_ENGINE_DENSE_NONLEADER. */
int jg_step_dense_acks(jg_engine* e, const uint64_t* acks_host);
int jg_step_dense_acks_device(jg_engine* e, const uint64_t* acks_dev);
/* `n_ticks` consecutive dense ticks in one launch: tick t reads the [R][G] block at
 * acks_dev + t*R*G.  Identical in effect to n_ticks calls of jg_step_dense_acks_device;
 * the groups' state is read and written once per launch instead of once per tick. */
int jg_step_dense_acks_device_n(jg_engine* e, const uint64_t* acks_dev, uint32_t n_ticks);
/* The same for every shard of a multi-device engine: acks_dev[d] is shard d's own [n_ticks][R][G_d]
 * block in the memory of its device (G_d = its n_groups).  One launch per shard, issued by the
 * shard's host thread on the shard's stream; returns when all are enqueued. */
int jg_step_dense_acks_shards(jg_engine* e, const uint64_t* const* acks_dev, uint32_t n_ticks);

/* ---- dense node tick: the steady-state traffic of a cluster in column form ----------------
 * What a leader sends its followers on a Tick (leader.rs:234-245: heartbeat() if due, then
 * replicate()) and what they answer (follower.rs:130-217), as device-resident SoA mailboxes, so
 * that a whole protocol round of millions of groups never leaves HBM: one engine's outbox
 * columns are another engine's inbox columns (same device: the same pointers).
 *
 * Mailbox vocabulary (everything else a step emits is queued as ordinary jg_msg_row rows,
 * drained with jg_drain_messages, in per-group emission order).  One 8-byte word per message where
 * the message has one addressee, so that a tick touches as few address streams as possible (the node
 * tick is bound by the number of its memory instructions, not by their bytes: profiles/README.md):
 *   Heartbeat{term, commit, leader_id}      -> beat[g] = {term, commit}
 *   AppendEntries{term, leader_id, blocks}  -> beat[g].term, ae[r][g] = JG_AE(from, n): the blocks are
 *       ids from+1 .. from+n, each with next = id-1 — expressible exactly when the leader's chain is
 *       a run (the id set is [0, top] and every block's parent its predecessor: what append builds -
 *       and what a restarted replica re-opens, its head at its commit index possibly BELOW the top,
 *       chain.rs:117-137; replicate() ranges over the stored keys, leader.rs:135,152-157); a leader
 *       whose chain is not sends all messages of its Tick as rows instead
 *   AppendResponse{node_id, head}           -> answer[g], bits 63..8 (one word of the leader's inbox block)
 *   HeartbeatResponse{commit, has_committed}-> answer[g], bits 7..0 = has_committed; commit -> hb_commit[g]
 * Block ids in mailbox words are 56 bits wide: a group whose head reaches JG_MAILBOX_NONE raises
 * JG_FAULT_ENGINE_MAILBOX_RANGE instead of emitting (never silently wrong; sequential ids get there
 * after 7 x 10^16 appends).
 * FSM instructions are not queued by dense steps: they are the per-group commit / head deltas
 * (follower: Apply for keys [commit_before, commit_after), follower.rs:204; leader: as
 * jg_step_dense_acks). */
#define JG_AE_NONE 0xFFu /* low byte of an ae word: no AppendEntries for this slot / group this tick */
#define JG_HB_NONE 0xFFu /* low byte of an answer word: no HeartbeatResponse                        */
#define JG_MAILBOX_NONE 0x00FFFFFFFFFFFFFFull /* bits 63..8 of an answer word: no AppendResponse    */
/* (the all-ones word JG_NO_ACK is therefore "nothing at all" in both kinds of word) */
#define JG_ANSWER(ack_head, hb_code) (((uint64_t)(ack_head) << 8) | (uint64_t)(hb_code))
#define JG_AE(from, n) (((uint64_t)(from) << 8) | (uint64_t)(n))

typedef struct jg_leader_beat { /* what every follower of the group reads of the leader's Tick */
  uint64_t term;      /* current_term of this tick's messages                              */
  uint64_t hb_commit; /* Heartbeat.commit, or JG_NO_ACK: no heartbeat (not due / no leader) */
} jg_leader_beat;

typedef struct jg_leader_inbox { /* device pointers; answers == NULL: nothing came in */
  const uint64_t* answers;   /* [R][G] JG_ANSWER(AppendResponse.head or JG_MAILBOX_NONE, has_committed or
                                JG_HB_NONE) of slot r; own slot: JG_ANSWER(#ClientRequests to append, JG_HB_NONE),
                                the count as in jg_step_dense_acks                                          */
  const uint64_t* hbr_commit;/* [R][G] HeartbeatResponse.commit (read only where has_committed == 0)     */
} jg_leader_inbox;

typedef struct jg_leader_outbox { /* device pointers, all required */
  jg_leader_beat* beat; /* [G]                                                                        */
  uint64_t* ae;         /* [R][G] JG_AE(range start key = progress head of slot r, number of blocks
                           0..JG_MAX_INFLIGHT) (leader.rs:135,152), or JG_NO_ACK: nothing for slot r.
                           Row [own slot] is nobody's mail: while every group of the engine has the same
                           own slot (the default; jg_set_self_slots with one value) the kernel does NOT
                           write it - fill it with JG_NO_ACK once if something walks all R rows (the
                           engine's own blocks - jg_dense_cluster, jg_step_node - are filled that way) */
} jg_leader_outbox;

typedef struct jg_follower_inbox { /* device pointers */
  const uint32_t* leader;   /* [G] sender NodeId per group, or NULL: `leader_id` for every group   */
  uint32_t leader_id;
  uint32_t reserved;
  const jg_leader_beat* beat;/* [G] the leader's outbox beat                                        */
  const uint64_t* ae;       /* [G] this node's row of the leader's outbox ae                       */
} jg_follower_inbox;

typedef struct jg_follower_outbox { /* device pointers, all required */
  uint64_t* answer;    /* [G] JG_ANSWER(AppendResponse.head or JG_MAILBOX_NONE, has_committed or JG_HB_NONE):
                          this node's row of the leader's inbox answers                                 */
  uint64_t* hb_commit; /* [G] HeartbeatResponse.commit (written where a HeartbeatResponse is)          */
} jg_follower_outbox;

/* Leader half of a node tick.  Per group that is a healthy leader, in this order:
 *   1. the HeartbeatResponses of `in`, ascending slot (leader.rs:222-231: replicate() again if
 *      !has_committed && commit > 0 — those extra AppendEntries are queued as rows);
 *   2. the appends and AppendResponses of in->answers exactly as jg_step_dense_acks;
 *   3. if `out` != NULL: Command::Tick (leader.rs:234-245) into the outbox columns.
 * Groups that are not leaders ignore 1-2 as the reference does and are not ticked here
 * (jg_step_dense_follower ticks them): their outbox entries are "none". */
int jg_step_dense_leader(jg_engine* e, uint64_t now_ms, const jg_leader_inbox* in, const jg_leader_outbox* out);

/* Follower half of a node tick.  Per group that is not a leader, in this order:
 *   1. Heartbeat{beat.term, beat.hb_commit, leader}    if beat[g].hb_commit != JG_NO_ACK (follower.rs:178-217)
 *   2. AppendEntries{beat.term, leader, blocks}        if ae[g] != JG_NO_ACK             (follower.rs:130-176)
 *   3. Command::Tick                                   if tick != 0     (follower.rs:121-128, candidate.rs:48-68)
 * Leaders apply 1-2 as the reference does (leader.rs:200-208,263) and are not ticked here: the leader half ticks
 * whoever is a leader when the round begins - also one that steps down in 1-2 (one Tick per group and round).
 * Equivalent to submitting those commands through jg_submit/jg_step, except that
 * AppendResponse / HeartbeatResponse go to the outbox columns and no FSM rows are queued. */
int jg_step_dense_follower(jg_engine* e, uint64_t now_ms, const jg_follower_inbox* in,
                           const jg_follower_outbox* out, int tick);

/* ---- a node's whole tick from host rows: the dense kernels behind the Apply surface ---------------
 * What server::event_loop (src/raft/server.rs:103-165) does between two ticks of its interval, for
 * every partition this node hosts at once: apply whatever tcp_rx / client_rx delivered, one command at a
 * time IN THE ORDER IT ARRIVED (jg_submit: the rows of a partition in their stream order, partitions
 * interleaved in any way, no sorting on the host), then Command::Tick.  The result - state, faults, and per
 * partition the sequence of everything pushed on fsm_tx and rpc_tx - is that of jg_submit + jg_step over the
 * same rows followed by a Tick row per partition: Apply::apply in arrival order (mod.rs:471-479).  Nothing is
 * re-ordered.  The rows are uploaded as they are and classified on the device.  A partition whose rows all fit
 * the mailbox vocabulary -
 *     at most one AppendResponse and one HeartbeatResponse per member slot (heads < JG_MAILBOX_NONE),
 *     at most one ClientRequest, and only if this node leads the partition,
 *     at most one Heartbeat and one AppendEntries, only if this node does NOT lead the partition (a leader
 *     answers them with a role change or not at all, leader.rs:200-208,263), from the same sender with the
 *     same term, the Heartbeat first (one answer word holds HeartbeatResponse, AppendResponse in that order),
 *     the AppendEntries' blocks a run (ids consecutive, each block's parent its predecessor, <= 254 blocks)
 * - is served in column form by the dense node tick (the HBM-bound kernels).  A column forgets the order of
 * the rows that filled it; what of that order can matter travels with the columns: which AppendResponses
 * arrived BEFORE the ClientRequest (they met the chain head before the append: chain.rs:197-202 holds them to
 * it, and what they committed precedes the Notify on fsm_tx), and for every partition the lag-space tick does
 * not serve (a HeartbeatResponse without the commit makes the leader replicate() on the progress as it is at
 * that moment, leader.rs:222-231; forged or far-behind heads) the arrival index of every row: those are
 * replayed one command at a time in arrival order.  Every row of any OTHER partition (votes, Timeout, Restart,
 * explicit Tick rows, duplicates, a ClientRequest at a non-leader, ...) is applied by the general state machine
 * exactly as jg_submit + jg_step would (stream order); that partition then takes part in the Tick like
 * everybody else.  `rows_general` counts those rows: a matter of cost, never of results.
 * A column handed out by jg_node_inbox_columns stands for that peer's answers AFTER the step's rows, per
 * partition HeartbeatResponse then AppendResponse, slots ascending.
 *
 * Outputs: rpc_tx - the Tick's Heartbeat / AppendEntries and the followers' answers as the mailbox
 * columns of jg_node_outbox (pinned host memory, one copy per column), everything else as rows through
 * jg_drain_messages.  Per partition the reference's emission order is: where an answer word is set - the
 * ClientRequest rows of the step (the queue the Heartbeat flushed, follower.rs:190-197), the word's
 * HeartbeatResponse, its AppendResponse, then the partition's other rows (what its Tick sent); elsewhere - the
 * partition's rows (a leader's extra AppendEntries of apply_heartbeat_response), then the Tick's words:
 * Heartbeat, AppendEntries by ascending slot.  fsm_tx - unlike the plain dense entry points, jg_step_node
 * QUEUES the FSM rows of its dense halves for jg_drain_applies, run-length encoded per partition and step, in
 * emission order: the Apply range (JG_FSM_APPLY_LEADER range(a..=b).skip(1)) committed by the
 * AppendResponses that arrived before the ClientRequest, the JG_FSM_NOTIFY {a = block id, b = the
 * ClientRequest's token}, the Apply range of the self-ack and the AppendResponses after it; a follower: one
 * JG_FSM_APPLY_FOLLOWER range(a..b) - consecutive ranges concatenate exactly (the progress heads only
 * grow).  Faults: jg_drain_faults. */
enum {
  JG_NODE_LEADER_HALF = 1u,   /* serve the partitions this node leads (jg_step_dense_leader)            */
  JG_NODE_FOLLOWER_HALF = 2u, /* serve the partitions it follows (jg_step_dense_follower)              */
  JG_NODE_TICK = 4u,          /* Command::Tick for every partition after its rows (server.rs:125)      */
  /* No synchronisation inside the call: it returns as soon as everything is ENQUEUED - uploads, classification, the
   * dense halves, the downloads of the outbox columns - and the engine's pinned input columns (jg_submit_reserve) are
   * a second set from then on, so that the next tick can be decoded while this one runs.  The dense halves of such a
   * step leave the partitions whose rows take the general path alone; the step is SETTLED by the next call that looks at
   * the engine (jg_node_outbox_view first of all; any step, drain, read or jg_sync): the row count has landed by then,
   * and if it is not zero those rows are applied and the halves come back for exactly those partitions - the same
   * results and the same record order as the synchronous step, one pass later.  Single-device engines or shards. */
  JG_NODE_ASYNC = 8u,
  /* The Tick's AppendEntries words as ONE word per partition where every addressee's word is the same (the steady state:
   * every follower acknowledged the same head): jg_node_outbox.aec[g] is that word - JG_NO_ACK: nothing for anybody -
   * or JG_AEC_INDIVIDUAL: the words are in jg_node_outbox.ae (valid for exactly those partitions: they differ by addressee,
   * or the partition's rows took the general path in this step), which is
   * NULL - and is not downloaded: 8 bytes per partition instead of 8 (R - 1) - when no partition of the step needs it
   * (jg_node_outbox_view fetches the rows when one does).  Single-device engines or shards.
   * WHICH partitions read JG_AEC_INDIVIDUAL is a matter of representation, not of results (the engine marks every
   * partition whose rows took the general path; the oracle library reports the common word wherever the R - 1 words
   * agree): compare aec / ae between backends only after expansion (BatchedRaft::expand_columns). */
  JG_NODE_COMMON_AE = 16u,
  /* A leader partition's fsm_tx rows of the step as one JG_FSM_LEADER_STEP row where the step appended a block and the
   * commit index is within 255 of it (24 bytes instead of 48 or 72; other partitions: the plain rows as before). */
  JG_NODE_FSM_FUSED = 32u,
  /* TWO STEPS IN FLIGHT (with JG_NODE_ASYNC; single-device engines or shards): the step keeps its outputs - the outbox
   * columns and every fsm_tx / rpc_tx row and fault it produced - in a set of its own until its outbox has been VIEWED,
   * and the next such step may be taken before that: while the device runs step t + 1 and its inputs travel up, step t's
   * outputs travel home (server.rs:103-165's channels are asynchronous: what a tick pushed on fsm_tx / rpc_tx is
   * consumed while the loop already takes the next messages).  With kept steps outstanding
   *   - jg_node_outbox_view serves the OLDEST one: it waits for that step's outputs only (never for the newer step),
   *     and makes exactly that step's rows - in the order a synchronous step would have queued them - what the next
   *     jg_drain_applies[_view] / jg_drain_messages[_view] / jg_drain_faults deliver; the pointers of the view stay
   *     valid until the second next kept step begins;
   *   - at most TWO may be outstanding: a third jg_step_node is JG_EINVAL, and so is any other stepping call
   *     (jg_step, a step without this flag, the dense entry points) - view the outboxes first;
   *   - reads (jg_read_state, jg_sync, counters) see the engine after the newest step.
   * The step's fsm rows come home behind its own kernels, the copy sized from the step before (no drain is issued by
   * the host, nothing waits for a count); rows of the general path, exceptional rows and faults - none in the steady
   * state - are collected when the outbox is viewed.  Same results, same rows, same order per step as without the flag. */
  JG_NODE_KEEP = 64u
};
#define JG_AEC_INDIVIDUAL 0xfffffffffffffffeull /* jg_node_outbox.aec: "see the rows of ae" (no JG_AE word: a range start stays below JG_MAILBOX_NONE) */
typedef struct jg_node_outbox { /* host pointers into the engine's pinned buffers; NULL: that half did not run */
  const jg_leader_beat* beat;  /* [G]    what a leader's followers read of its Tick (jg_leader_outbox.beat)   */
  const uint64_t* ae;          /* [R][G] JG_AE(from, n) per addressee slot, JG_NO_ACK: none (JG_NODE_COMMON_AE: see there) */
  const uint64_t* answer;      /* [G]    JG_ANSWER(AppendResponse.head, has_committed) to the partition's leader */
  const uint64_t* hb_commit;   /* [G]    HeartbeatResponse.commit (valid where the answer carries a response)  */
  uint64_t rows;               /* command rows the step took                                                   */
  uint64_t rows_general;       /* ... of which went through the general state machine                          */
  uint64_t bytes_h2d;          /* PCIe: uploaded for this step                                                 */
  uint64_t bytes_d2h;          /* PCIe: outbox columns downloaded for this step (drains not included)          */
  const uint64_t* aec;         /* [G]    JG_NODE_COMMON_AE: the partition's AppendEntries word for every addressee, else NULL */
} jg_node_outbox;
/* Column inbound for jg_step_node: a peer that is itself a batched engine ships its followers' answers as the
 * column it produced (jg_node_outbox.answer / .hb_commit) instead of two rows per partition.  The call hands out
 * where member slot `slot`'s column lives in the engine's pinned memory - *answer: [G] JG_ANSWER words (JG_NO_ACK:
 * nothing from that peer for the partition), *hb_commit: [G] HeartbeatResponse.commit (read only where the word
 * carries has_committed == 0); the caller fills them IN PLACE before the next jg_step_node, whose leader half applies
 * them for EVERY partition (after that step's general-path rows), exactly as if each word had been an
 * AppendResponse / HeartbeatResponse row of a column-form partition.  hb_commit == NULL: the commit is 0 for every
 * has_committed == 0 response of the column (not uploaded).  The hand-out covers ONE step.  `slot` must not be the
 * own slot of any partition (that word carries the append count), and a ROW of the same step that names the same
 * sender is an error (JG_EINVAL at the next synchronising call): a peer speaks columns or rows within one tick.
 * Single-device engines (or a shard's own handle). */
int jg_node_inbox_columns(jg_engine* e, uint32_t slot, uint64_t** answer, uint64_t** hb_commit);

/* Apply everything queued by jg_submit since the last step as described above (`flags`: JG_NODE_*; at
 * least one half).  Asynchronous like jg_step except for one synchronisation after the classification
 * (the number of general-path rows sizes that step's launch) - none at all with JG_NODE_ASYNC. */
int jg_step_node(jg_engine* e, uint64_t now_ms, uint32_t flags);
/* The mailbox columns the last jg_step_node produced: waits for them to land; the pointers stay valid
 * until the next jg_step_node.  On a multi-device engine the columns are the shards' concatenated.
 * (JG_NODE_KEEP: the OLDEST step whose outbox has not been viewed - see there.) */
int jg_node_outbox_view(jg_engine* e, jg_node_outbox* out);

/* ---- a poll behind a kept node step: the feeds with two ticks in flight (ABI v21) --------------------
 * jg_engine_poll and the separate feed calls are refused while kept node steps are outstanding: between
 * two steps whose outputs are not due a synchronous answer has no place.  In a loop that always has a
 * step outstanding (JG_NODE_ASYNC | JG_NODE_KEEP, two ticks in flight) that is every tick.  A POLLED step
 * carries its poll with it: queued behind the step's own kernels, it sees the engine exactly as that step
 * leaves it, travels home on the step's own trip and is handed out when that step's outbox is viewed.
 * Nothing is synchronised that jg_step_node with JG_NODE_KEEP does not synchronise.  It defines no value
 * of its own:
 *
 * CONTRACT.  Let S be the engine after step t is settled and before anything else touches it.  The answer
 * viewed for step t is what jg_engine_poll with the same jg_poll leaves when called on S: every row byte,
 * every total, the backlog and both censuses; and the three shadows and the replication clocks are
 * afterwards what that call leaves - JG_WATCH_PEEK counts per feed as there, and under the time rule the
 * clocks of every slot of the range advance to clock->now_ms whatever the cap, unless the replicas part
 * peeks.  Consecutive polled steps are consecutive polls: what a small cap leaves pending at step t is
 * pending at step t + 1.  A kept step without a poll leaves the feeds alone.  jg_engine_poll and the
 * separate feed calls stay refused while kept steps are outstanding; once none is they may be mixed with
 * polled steps on one engine - one set of shadows, one set of clocks.
 *
 * jg_step_node_polled is jg_step_node(e, now_ms, flags) with *request attached.  request == NULL is
 * exactly jg_step_node.  Otherwise flags must contain JG_NODE_KEEP (and so JG_NODE_ASYNC) and `e` must not
 * be a multi-device parent (JG_NODE_KEEP is per shard already).  *request and, if JG_POLL_REPLICAS is
 * wanted and clock != NULL, *request->clock are copied at entry.  READ are the input fields: want, g0, n,
 * the three flag words, policy, census_lag_limit, clock and the three *_cap fields.  The output pointers
 * are never written through: backlog != NULL only says "the backlog is wanted", the row and census
 * pointers are ignored.  Every argument is checked by jg_engine_poll's own rules before anything of the
 * step is queued: a refused call (JG_EINVAL) steps nothing and leaves the submitted rows queued.
 *
 * jg_node_poll_view answers for the kept step whose outbox jg_node_outbox_view finished last; JG_EINVAL if
 * no kept step has been viewed yet.  want == 0: that step carried no poll (JG_OK, everything else 0).  The
 * rows live in the engine's pinned memory, one landing area per kept-step set, and stay valid as long as
 * that view's outbox columns do: until the next node step claims the set.  Each feed's rows come home
 * behind the step, the copy sized from the polled step finished last; what is missing is fetched when the
 * step is viewed.
 *
 * A step whose rows took the general path is completed by a catch-up pass when it is settled.  The poll
 * queued behind such a step's first pass finds that out on the device (the step's general-row count) and
 * writes neither shadow nor clock; the same request is queued once more behind the catch-up pass, and
 * `state` says so: JG_NODE_POLL_REDONE, informational - the answer is S's either way. */
enum { JG_NODE_POLL_REDONE = 1u };    /* jg_node_poll.state */
typedef struct jg_node_poll {
  uint32_t want, state;               /* the request's want (0: the step carried no poll); JG_NODE_POLL_*   */
  const jg_leader_row* leaders;       /* [leaders_n], ascending; _n = min(cap, total)                       */
  size_t leaders_n, leaders_total;
  const jg_isr_row* replicas;
  size_t replicas_n, replicas_total;
  const jg_commit_row* commits;
  size_t commits_n, commits_total;
  jg_commit_backlog backlog;          /* zero unless wanted                                                 */
  jg_census census;
  jg_repl_census repl_census;
} jg_node_poll;
int jg_step_node_polled(jg_engine* e, uint64_t now_ms, uint32_t flags, const jg_poll* request);
int jg_node_poll_view(jg_engine* e, jg_node_poll* out);

/* ---- completions behind a kept node step (ABI v23) ------------------------------------------------
 * The completion feed's three calls are refused while kept steps are outstanding, like every feed's.
 * An AWAITED step carries a registration and a watch with it, as a polled step carries its poll.
 *
 * CONTRACT.  Let S be the engine after kept step t is settled and before anything else touches it.  The
 * answer viewed for step t is what jg_engine_await_blocks(e, rows, n), then (ABI v24, cancel_n != 0)
 * jg_engine_await_cancel(e, cancel_keys, cancel_n, cancel_mask, &marked) and then
 * jg_engine_watch_completions(e, flags, now_ms, out, cap, &total, &stats) leave when called on S: every
 * row byte, total, all six stat words, marked; and the table afterwards holds the same waiters in the same
 * order.  Rows registered by the step can be withdrawn by its own cancel.
 * Consecutive awaited steps are consecutive register-then-watch pairs: what a small cap leaves pending at
 * step t is pending at step t + 1.  A kept step without the attachment leaves the table alone.  The
 * three synchronous calls stay refused while kept steps are outstanding; once none is they may be mixed
 * with awaited steps on one engine - there is one table.
 *
 * jg_step_node_awaited with await == NULL is exactly jg_step_node_polled(e, now_ms, flags, poll).
 * Otherwise the polled step's rules hold (JG_NODE_ASYNC | JG_NODE_KEEP, no multi-device parent), *await
 * its rows and its cancel keys are copied at entry, and every argument is checked by the rules of
 * jg_engine_await_blocks, jg_engine_await_cancel and jg_engine_watch_completions - and `poll`, if not
 * NULL, by jg_engine_poll's - before anything of the step is queued: a refused call steps nothing and
 * leaves the submitted rows queued.  The poll, if both are attached, is queued first.
 *
 * CAPACITY.  With steps outstanding the host does not know how many waiters the table holds; it keeps a
 * BOUND: the waiters outstanding as of the newest viewed step or synchronous call, plus every row
 * registered by steps begun since then.  bound + n > capacity: JG_ECAPACITY, nothing is stepped.  (What
 * an outstanding step's watch removes lowers the bound when that step is viewed, not before.)
 *
 * jg_node_await_view answers for the kept step whose outbox jg_node_outbox_view finished last; JG_EINVAL
 * if no kept step has been viewed yet.  attached == 0: that step carried no request (JG_OK, everything
 * else 0).  The rows live in the set's pinned landing area and stay valid as long as that view's outbox
 * columns do.  state: JG_NODE_POLL_REDONE as for the poll - the step had general-path rows, the chain
 * behind its first pass touched nothing (the device saw the count) and ran behind the catch-up pass. */
typedef struct jg_node_await_request {
  const jg_await_row* rows;           /* [n] registered first; n == 0: watch only                          */
  size_t n;
  uint32_t flags;                     /* 0 or JG_WATCH_PEEK                                                 */
  uint32_t want_stats;                /* 0 / 1                                                              */
  uint64_t now_ms;                    /* != UINT64_MAX                                                      */
  size_t cap;                         /* rows the caller takes; 0: counts only                              */
  const uint64_t* cancel_keys;        /* [cancel_n] jg_engine_await_cancel between the two (ABI v24)        */
  size_t cancel_n;                    /* 0: no cancel                                                       */
  uint64_t cancel_mask;
} jg_node_await_request;
int jg_step_node_awaited(jg_engine* e, uint64_t now_ms, uint32_t flags, const jg_poll* poll /* may be NULL */,
                         const jg_node_await_request* await /* may be NULL */);
typedef struct jg_node_await {
  uint32_t attached, state;           /* 1: the step carried a request; JG_NODE_POLL_REDONE                 */
  const jg_done_row* rows;            /* [rows_n], registration order; rows_n = min(cap, total)             */
  size_t rows_n, total;
  jg_await_stats stats;               /* zero unless wanted                                                 */
  size_t marked;                      /* the waiters the step's cancel newly marked (ABI v24)               */
} jg_node_await;
int jg_node_await_view(jg_engine* e, jg_node_await* out);

/* ---- point queries behind a kept node step (ABI v25) ----------------------------------------------
 * jg_engine_lookup_groups is refused while kept steps are outstanding, like every call that reads.  A
 * LOOKED step carries a point query with it, as a polled step carries its poll and an awaited step its
 * completion request: the state of exactly these partitions - leader, term, head, commit, the progress
 * heads - without a bubble in a loop that always has a step outstanding.
 *
 * CONTRACT.  Let S be the engine after kept step t is settled and before anything else touches it.  The
 * answer viewed for step t is what jg_engine_lookup_groups(e, lookup, rows, match) writes when called on
 * S: every byte of every row and every progress head.  The call defines no value of its own.  It reads
 * state columns only: it writes no shadow, clock, table or column of the state machine, and a kept step
 * with or without a lookup leaves every other result unchanged - the step's outbox, its drains, its poll
 * and its completions.  jg_engine_lookup_groups itself stays refused while kept steps are outstanding;
 * once none is the two may be mixed freely.
 *
 * jg_step_node_looked with lookup == NULL is exactly jg_step_node_awaited(e, now_ms, flags, poll, await).
 * Otherwise the polled step's rules hold (JG_NODE_ASYNC | JG_NODE_KEEP, no multi-device parent), and
 * *lookup and its host list are copied at entry: the caller's memory is free when the call returns.
 * Accepted: a range (groups == NULL: g0, n) or a host list (unsorted, repeats allowed), optionally
 * JG_LOOKUP_PROGRESS.  Refused with JG_EINVAL: JG_GROUPS_DEVICE (a device list's bounds are known only
 * on the device, and a refusal that arrives a tick late is not worth having), n > JG_NODE_LOOKUP_MAX, an
 * index >= G, a range out of bounds, a non-null self_slots, an unknown flag.  Every argument - `poll`
 * and `await` by their own rules - is checked before anything of the step is queued: a refused call
 * steps nothing and leaves the submitted rows queued.  n == 0 is an attached lookup with no rows.  The
 * poll and the completion request, if attached, are queued first.
 *
 * jg_node_lookup_view answers for the kept step whose outbox jg_node_outbox_view finished last; JG_EINVAL
 * if no kept step has been viewed yet.  attached == 0: that step carried no lookup (JG_OK, everything
 * else 0).  The rows and the progress heads live in the set's pinned landing area (sized at entry: n is
 * known, nothing is fetched later) and stay valid as long as that view's outbox columns do.  state:
 * JG_NODE_POLL_REDONE as for the poll - the step had general-path rows, the pass behind its first pass
 * wrote no row (the device saw the count) and ran once more behind the catch-up pass. */
#define JG_NODE_LOOKUP_MAX 65536u     /* entries a step can carry: one staging piece of jg_engine_lookup_groups */
int jg_step_node_looked(jg_engine* e, uint64_t now_ms, uint32_t flags, const jg_poll* poll /* may be NULL */,
                        const jg_node_await_request* await /* may be NULL */, const jg_group_set* lookup /* may be NULL */);
typedef struct jg_node_lookup {
  uint32_t attached, state;           /* 1: the step carried a lookup; JG_NODE_POLL_REDONE                  */
  const jg_group_state* rows;         /* [n], in the order asked                                            */
  size_t n;
  const uint64_t* match;              /* [n][R] progress heads, or NULL (JG_LOOKUP_PROGRESS not asked)      */
} jg_node_lookup;
int jg_node_lookup_view(jg_engine* e, jg_node_lookup* out);

/* ---- opening and closing partitions behind a kept node step (ABI v26) -----------------------------
 * jg_engine_open_groups and jg_engine_close_groups are refused while kept steps are outstanding or
 * commands are queued, like every call that rewrites group state.  A HOSTED step carries a hosting
 * request with it, as a polled step carries its poll, an awaited step its completion request and a looked
 * step its point query: LeaderAndIsr, CreateTopics, DeleteTopics and the last step of a partition move
 * without a bubble in a loop that always has a step outstanding - the next tick's rows may already
 * address the slots this tick opens.
 *
 * CONTRACT.  Let S be the engine after kept step t is settled and before anything else touches it.  A
 * step carrying a hosting request leaves the engine as jg_engine_close_groups(S, close) followed by
 * jg_engine_open_groups(., now_ms, open) would, with the step's own now_ms: every column of every slot,
 * the carried draw counts included.  The call defines no value of its own.  The two sets are independent,
 * as two synchronous calls are: a set the synchronous call would refuse for a slot's state (opening a
 * hosted slot, closing a vacant one) writes nothing, reports JG_NODE_HOSTING_CLOSE_REFUSED or
 * JG_NODE_HOSTING_OPEN_REFUSED with the step's view and does not affect the other set.  The open's check
 * sees the close's writes: a slot may be closed and reopened in one step.  The step's own outbox, drains,
 * poll, completions and lookup all see S: the hosting pass is the last thing behind the step.  The feeds
 * of step t + 1 see the change through the diff alone, as after the synchronous calls, and a waiter on a
 * closed slot leaves as JG_DONE_VACANT at the next watch.  Rows of step t addressed to a slot it closes
 * are applied first; rows of step t addressed to a slot it opens meet a vacant slot and are ignored; rows
 * of step t + 1, submitted before step t is viewed, meet the opened slot.  The synchronous calls stay
 * refused while kept steps are outstanding; once none is the two may be mixed freely.
 *
 * jg_step_node_hosted with hosting == NULL is exactly jg_step_node_looked(e, now_ms, flags, poll, await,
 * lookup).  Otherwise the polled step's rules hold (JG_NODE_ASYNC | JG_NODE_KEEP, no multi-device
 * parent), and both sets, their host lists and self_slots are copied at entry: the caller's memory is free
 * when the call returns.  Either set may be NULL.  Accepted per set: a range (groups == NULL: g0, n - any
 * length within G) or a host list, strictly ascending, of at most JG_NODE_HOSTING_MAX entries; on the open
 * set self_slots (with a list or a range of at most JG_NODE_HOSTING_MAX entries).  Refused with JG_EINVAL:
 * an unknown flag, JG_GROUPS_DEVICE (a device list's bounds are known only on the device, and a refusal
 * that arrives a tick late is not worth having), a longer list, an index >= G, a range out of bounds, a
 * list that is not strictly ascending, self_slots[i] >= R, self_slots on the close set.  Every argument -
 * `poll`, `await` and `lookup` by their own rules - is checked before anything of the step is queued: a
 * refused call steps nothing and leaves the submitted rows queued.  The state check (open needs vacant,
 * close needs hosted) is made on the device, behind the step, and arrives with the view: vacancy is the
 * device's knowledge.  A set with n == 0 is attached and writes nothing.  The poll, the completion request
 * and the lookup, if attached, are queued first.
 *
 * jg_node_hosting_view answers for the kept step whose outbox jg_node_outbox_view finished last;
 * JG_EINVAL if no kept step has been viewed yet.  attached == 0: that step carried no hosting request
 * (JG_OK, everything else 0).  closed / opened: the slots each set wrote - its n, or 0 when it was refused
 * (or NULL).  state: JG_NODE_POLL_REDONE as for the poll - the step had general-path rows, the passes
 * behind its first pass wrote nothing (the device saw the count) and ran once more behind the catch-up
 * pass - and the two *_REFUSED bits. */
enum { JG_NODE_HOSTING_MAX = 65536u }; /* entries of a host list (or of self_slots) a step can carry */
enum { JG_NODE_HOSTING_CLOSE_REFUSED = 2u, JG_NODE_HOSTING_OPEN_REFUSED = 4u }; /* jg_node_hosting.state, beside JG_NODE_POLL_REDONE */
typedef struct jg_node_hosting_request {
  const jg_group_set* close;          /* may be NULL: made first                                            */
  const jg_group_set* open;           /* may be NULL: made at the step's now_ms                             */
} jg_node_hosting_request;
typedef struct jg_node_hosting {
  uint32_t attached, state;           /* 1: the step carried a request; JG_NODE_POLL_REDONE, JG_NODE_HOSTING_*_REFUSED */
  uint32_t closed, opened;            /* slots written by each set: its n, or 0                             */
} jg_node_hosting;
int jg_step_node_hosted(jg_engine* e, uint64_t now_ms, uint32_t flags, const jg_poll* poll /* may be NULL */,
                        const jg_node_await_request* await /* may be NULL */, const jg_group_set* lookup /* may be NULL */,
                        const jg_node_hosting_request* hosting /* may be NULL */);
int jg_node_hosting_view(jg_engine* e, jg_node_hosting* out);

/* ---- a closed loop of dense node ticks ------------------------------------------------------------
 * All R nodes of every partition in ONE process (one engine per node, e.g. the three brokers of
 * examples/multi-node in one runtime): the protocol round — leader half on nodes[lead], follower half
 * on every other node, each one's outbox columns being the others' inbox columns — driven from
 * inside the library, so that a round costs its launches and no per-call host overhead of the
 * caller's language.  The cluster owns the mailbox columns (in the memory of nodes[lead]'s device);
 * nothing synchronises with the host inside a round.  While the cluster exists, the nodes that share
 * nodes[lead]'s device issue ALL their work on its stream (the halves of a round are bandwidth-bound:
 * side by side they only slow each other down); nodes on other devices keep their streams and are
 * chained with events.
 * Equivalent, call for call, to jg_step_dense_leader on nodes[lead] followed by jg_step_dense_follower
 * (tick = 1) on the others (josefine::DenseCluster::round in josefine_amd/host/raft_handle.hpp).
 * Engines are borrowed: destroy the cluster BEFORE them (it gives them their streams back). */
typedef struct jg_dense_cluster jg_dense_cluster;
/* lead = JG_CLUSTER_ANY_LEADER: PER-PARTITION LEADERSHIP - every node leads the partitions it was elected for and
 * follows the others (what a josefine cluster looks like after its elections: candidate.rs:101-113 -> leader.rs:124-174).
 * The mailbox columns are then the CLUSTER's, indexed by group and slot: whoever leads group g reads row r of the
 * answers as slot r's answer and writes the beat and the AppendEntries words of g; every other node reads its
 * word, follows and answers into its own row.  A round is
 *   0. the claim: owner[g] = the lowest slot whose node is a healthy leader of g (JG_OWNER: nobody);
 *   1. every node's leader half over the groups it leads - the owner's exactly as jg_step_dense_leader (its own slot's
 *      word = the ClientRequests jg_dense_cluster_set_appends offers to whoever owns g), its Tick into the columns;
 *      a leader that is NOT the owner (two terms' leaders in one round) gets no inbox and no ClientRequest, and its
 *      Tick travels as rows (Heartbeat rows are delivered by the routed round's transport, AppendEntries rows stay
 *      queued for the host like every AppendEntries row);
 *   2. every node's follower half over the groups it does not lead, tick = 1, sender = the owner's NodeId - mail only
 *      where somebody else owns the group.
 * Equivalent, call for call, to that sequence of jg_step_dense_leader / jg_step_dense_follower calls with the inboxes
 * masked accordingly (tests/dense_node.py::AnyLeaderCluster states it in numpy).  Each node takes two steps per round.
 * The nodes must share a device; n_nodes <= 6; nodes[r] hosts replica slot r of every group. */
#define JG_CLUSTER_ANY_LEADER 0xFFFFFFFFu
int jg_dense_cluster_create(jg_engine* const* nodes, uint32_t n_nodes, uint32_t lead, jg_dense_cluster** out);
void jg_dense_cluster_destroy(jg_dense_cluster* c);
/* Per-cluster options (fixed before the cluster's first routed round; JG_EINVAL afterwards or for an unknown option).
 *   JG_CLUSTER_OPT_VOTE_WORDS (0 / 1): jg_dense_cluster_round_routed moves an ELECTION's traffic - a campaign's
 *     VoteRequest broadcasts (candidate.rs:24-45) and the VoteResponses they are answered with (follower.rs:219-246,
 *     candidate.rs:66-113) - as mailbox words per (partition, sender) read by a dense receiving half instead of as rows
 *     through the row transport, wherever EVERYTHING a node receives for a partition in a round is such traffic; what the
 *     nodes compute, emit and keep for the host is the row transport's, bit for bit (jg_route_stats.delivered counts rows
 *     only and is smaller).  Needs nodes that share the cluster's stream (one device) and R >= 2; otherwise ignored. */
enum { JG_CLUSTER_OPT_VOTE_WORDS = 1 };
int jg_dense_cluster_set_option(jg_dense_cluster* c, uint32_t option, uint64_t value);
/* ClientRequests every group appends per round (leader.rs:177-197): the same number for all groups,
 * or (per_group != NULL) one value per group from host memory.  (JG_CLUSTER_ANY_LEADER: offered to whoever owns the
 * group that round; a group nobody leads is offered nothing.) */
int jg_dense_cluster_set_appends(jg_dense_cluster* c, uint64_t uniform, const uint64_t* per_group);
/* No more ClientRequests for the n groups listed in DEVICE memory (ascending or not; duplicates allowed): their
 * offered count becomes 0 from the next round on - a client that has lost its partition's leader stops proposing
 * (what the reference makes of a re-elected leader is Q8: its first append panics, chain.rs:163).  Asynchronous on the
 * cluster's stream; the list must stay valid until then (jg_sync). */
int jg_dense_cluster_withdraw_appends(jg_dense_cluster* c, const uint32_t* groups_dev, uint32_t n);
/* ... and `per_round` ClientRequests per round for them from the next round on (0: withdraw) - the client proposes again to
 * partitions that were re-created (JG_CMD_RECREATE) and have a leader that can append.  Same conventions. */
int jg_dense_cluster_offer_appends(jg_dense_cluster* c, const uint32_t* groups_dev, uint32_t n, uint64_t per_round);
/* n_rounds protocol rounds at logical times now_ms, now_ms + dt_ms, ...; asynchronous (jg_sync the nodes).  Two or more
 * rounds are replayed as captured graphs (logical time and step numbers live in a device-resident clock that advances
 * itself), eight rounds to a graph where n_rounds allows; the results are those of n_rounds calls with one round each. */
int jg_dense_cluster_rounds(jg_dense_cluster* c, uint64_t now_ms, uint64_t dt_ms, uint32_t n_rounds);
/* The mailbox columns, for inspection: the leader's inbox / outbox as the structs above.  out->ae is a SNAPSHOT of the
 * last round's AppendEntries words, written out at this call (the cluster keeps ONE word per group where every follower's
 * is the same: JgLeaderNode::o_aec) and valid until the next round; with JG_CLUSTER_ANY_LEADER the rows of a group nobody
 * owns read JG_NO_ACK. */
int jg_dense_cluster_mailboxes(jg_dense_cluster* c, jg_leader_inbox* in, jg_leader_outbox* out);

/* One protocol round WITH a transport for everything outside the mailbox vocabulary — elections above
 * all: in the reference a VoteRequest leaves on rpc_tx, crosses tcp.rs and comes back out of the peer's
 * event loop as a Command (server.rs:127-137); here the rows the nodes queued during the round are
 * taken out of their undrained output ON THE DEVICE and become the addressees' first step of the next
 * routed round.  Per node and call:
 *   1. jg_step over the rows delivered by the previous call, then over inject[node] (a device batch as
 *      for jg_step_device_rows, or n == 0; NULL = nothing for anybody) — per group: the peers' rows in
 *      the order (phase of the round they were emitted in, emission index within the sender's step,
 *      sender slot), then the injected ones.  The phases are the steps the nodes take in lockstep: 1 = this
 *      step over the delivered rows, 2 = the injected rows, 3 = the leader half, 4 = the follower half of the
 *      dense round.  Every sender's stream arrives in its own order - all a network promises (one
 *      connection per peer pair, tcp.rs:87-170) - and the senders are interleaved: everybody's first row of a
 *      phase before anybody's second.  That interleaving is what lets an election of more than three nodes
 *      complete: a candidate broadcasts its VoteRequest once per peer (candidate.rs:30-37), a voter grants
 *      the first copy and refuses the rest, and a voter's later answer overwrites its earlier one
 *      (election.rs:33-35) - the quorum has to be seen among the first answers.  (Until ABI v8 the order was
 *      sender-major, each sender's rows back to back: five-node elections could not be won.);
 *   2. the dense round of jg_dense_cluster_rounds at now_ms, except that the ClientRequests of
 *      jg_dense_cluster_set_appends are offered only to groups nodes[lead] leads at that moment (a
 *      replica without a leader queues them, follower.rs:258-270: not a dense append; with per-partition
 *      leadership: to whoever owns the group);
 *   3. the transport: rows addressed to members (JG_TO_PEERS: all other members; JG_TO_PEER: to_id)
 *      are delivered, EXCEPT AppendEntries rows (the payload is the sender's block store) and
 *      ClientRequest rows (instructions to the host adapter about its request mirror): those, and
 *      everything addressed elsewhere, stay queued for jg_drain_messages, as do FSM rows.
 * A sender whose round left nothing for the host needs no drain (its output regions are recycled).
 * The nodes must share a device.  Synchronises with the host once per call (row counts).  Arguments are checked
 * before anything is launched; an error after the round has begun to consume the delivered rows (a HIP failure,
 * an internal inconsistency) leaves messages lost in flight: the cluster is marked failed and every later call
 * returns JG_EDEVICE - destroy it. */
typedef struct jg_route_stats {
  uint64_t delivered[JG_MAX_REPLICAS]; /* rows queued for node n's next routed round                   */
  uint64_t kept;                       /* message rows of this round left for jg_drain_messages        */
  uint64_t fsm_rows;                   /* FSM rows this round's steps queued (jg_drain_applies)        */
} jg_route_stats;
int jg_dense_cluster_round_routed(jg_dense_cluster* c, uint64_t now_ms, const jg_cmd_batch* inject /* [n_nodes] or NULL */,
                                  jg_route_stats* stats /* may be NULL */);

/* Batched Chain::compact (src/raft/chain.rs:239-253) as a pure function over
 * explicit (id,next) trees: tree t owns entries [off[t], off[t+1]); ids within a
 * tree need not be sorted.  removed[i] = 1 iff the walk removes entry i. */
int jg_chain_compact(jg_engine* e, size_t n_trees, const uint64_t* off /*[n_trees+1]*/,
                     const uint64_t* ids, const uint64_t* nexts, const uint64_t* commits /*[n_trees]*/,
                     uint8_t* removed /* [off[n_trees]] out */);

/* Chain::compact (src/raft/chain.rs:239-253, incl. its quirk Q7: the parent pointer of a REMOVED
 * block is followed too) on the resident chain of every healthy group: the blocks below the
 * commit index that the walk removes leave the engine's id set, and are queued as rows for the
 * host to delete from its block store (jg_drain_compacted: group ascending, ids descending = the
 * order of the walk).  *n_removed (optional) = rows this call queued.  The reference never calls
 * compact() outside its test; a host that wants its dead branches gone calls this between steps. */
typedef struct jg_compact_row {
  uint32_t group;
  uint32_t pad;
  uint64_t id; /* BlockId removed from the chain of `group` */
} jg_compact_row;
int jg_chain_compact_resident(jg_engine* e, size_t* n_removed);
int jg_drain_compacted(jg_engine* e, jg_compact_row* out, size_t cap, size_t* n);

int jg_sync(jg_engine* e);

/* Device-side ordering between two engines of one process: everything `waiter` enqueues after
 * this call runs after everything `signal` has enqueued so far (hipEventRecord on signal's
 * stream + hipStreamWaitEvent on waiter's; no host synchronisation).  What chains the dense
 * mailboxes of several engines — one engine's outbox columns are another's inbox. */
int jg_stream_wait(jg_engine* waiter, jg_engine* signal);

/* Drains.  Each returns the queued rows (per-group emission order identical to the
 * reference; groups in ascending order within one step) and clears the queue.
 * With out == NULL only *n is set. */
int jg_drain_messages(jg_engine* e, jg_msg_row* out, size_t cap, size_t* n);
int jg_drain_applies(jg_engine* e, jg_fsm_row* out, size_t cap, size_t* n);
int jg_drain_faults(jg_engine* e, jg_fault_row* out, size_t cap, size_t* n);
/* Zero-copy drains: *rows points at the engine's pinned host queue (filled by one
 * asynchronous device-to-host copy), valid until the next drain call on the SAME queue
 * (drains of the other queues, faults, steps and reads in between leave them alone; step
 * results are not affected: the rows count as drained).  What a Rust adapter iterates to
 * re-emit on rpc_tx / fsm_tx without an intermediate Vec. */
int jg_drain_messages_view(jg_engine* e, const jg_msg_row** rows, size_t* n);
int jg_drain_applies_view(jg_engine* e, const jg_fsm_row** rows, size_t* n);

/* Pipelined drains.  jg_drain_prefetch marks a point in the step stream and starts, without
 * blocking, the compaction and the transfer to the host queues of every row that steps before
 * the point have produced — on a second HIP stream behind an event, driven by the engine's own
 * drain thread, while the caller keeps stepping.  From the first call on the engine is PIPELINED:
 *   - jg_drain_prefetch never blocks: while a batch is still in transfer it starts nothing (the
 *     next call covers more steps);
 *   - the jg_drain_* calls never block and never synchronise with the step stream: they deliver the
 *     rows of the batches that have landed (same order as ever: steps in order, groups ascending
 *     within a step), possibly none;
 *   - jg_drain_wait blocks until the batch in transfer (if any) has landed - the back-pressure of a
 *     caller that does not want to run more than one batch ahead of its own output;
 *   - jg_drain_flush blocks until everything stepped so far has landed (then drain).
 * The pattern for a caller that forwards messages every N ticks (what server::event_loop does with
 * rpc_tx for one group, src/raft/server.rs:125-159):
 *     every N ticks: jg_drain_*_view (whatever has landed) ... jg_drain_prefetch (next batch)
 * so that PCIe time and host time of one batch overlap the device time of the following ticks. */
int jg_drain_prefetch(jg_engine* e);
int jg_drain_wait(jg_engine* e);
int jg_drain_flush(jg_engine* e);

/* Copy one state column for groups [g0, g0+n) to host memory (element type per
 * JG_FIELD_* above).  `replica` selects the slot for JG_FIELD_MATCH. */
int jg_read_state(jg_engine* e, int field, uint32_t replica, void* out, uint32_t g0, uint32_t n);

/* Counters since creation: [0] commands applied, [1] quorum decisions
 * (Leader::commit evaluations + election_status evaluations),
 * [2] group-steps of the dense path, [3] kernel launches (a dense ack tick counts once, also where the engine
 * issues it as two half-grids - see "device-resident helpers" below -, plus one for the general-path kernel
 * where that is scheduled behind it). */
int jg_get_counters(jg_engine* e, uint64_t out[4]);

/* ---- device-resident helpers for benchmarks ---------------------------------
 * The engine owns its stream; these let a caller keep inputs in HBM and time
 * the stream with HIP events without linking the HIP runtime itself.
 * Streams: between 1 M and 4 M groups (JG_DENSE_SPLIT_MIN in the environment at jg_engine_create: the lower end,
 * then with no upper end; 0: never) jg_step_dense_acks_device issues the tick as two launches, the second half of
 * the groups on a second stream the engine owns, and consecutive ticks of the two halves overlap.  Nothing of this
 * is visible through the API: every other call - steps, reads, drains, feeds, jg_sync, jg_stream_wait,
 * jg_timer_start / jg_timer_stop, the jg_device_* helpers - is ordered behind both halves and ahead of the next
 * tick's, and the engine is "idle" only when both streams are.  As before, the ack block of a device-pointer tick
 * must be complete when the call is made and must stay untouched until a later call on the engine has
 * synchronised (or been ordered behind the tick: anything issued through the engine is); a caller's own work on
 * another stream is neither waited for nor delayed. */
int jg_device_alloc(jg_engine* e, size_t bytes, void** dev_ptr);
int jg_device_free(jg_engine* e, void* dev_ptr);
int jg_device_upload(jg_engine* e, void* dev_dst, const void* host_src, size_t bytes);
int jg_device_download(jg_engine* e, void* host_dst, const void* dev_src, size_t bytes);
int jg_timer_start(jg_engine* e);            /* hipEventRecord on the engine stream */
int jg_timer_stop(jg_engine* e, float* ms);  /* record + synchronize + elapsed      */

/* Synthetic AppendEntries-ack stream generator,
 * counter-based so any shard regenerates its slice: fills one dense [R][G] tick
 * on the device from (seed, tick, global group, replica) and the generator's own
 * follower model kept in `sim` ([R][G] u64, zero-initialised by the caller).
 * mode 0: steady state (#3/#4) — 1 append per tick, every follower acks the
 *         leader head of the previous tick;
 * mode 1: ragged (#2) — a in {0,1,2} appends, follower ack = min(leader_head,
 *         prev_ack + U{0..MAX_INFLIGHT}), 5 % dropped, 5 % stale duplicates. */
int jg_synth_fill_acks_device(jg_engine* e, uint32_t mode, uint64_t tick, uint64_t* sim_dev,
                              uint64_t* acks_dev);

/* Measurement aid: HIP event pairs around the dense tick kernel itself (k_leader_tick_dense /
 * _n / k_leader_node_tick — not the k_dense_slow launch that may follow it), recorded on the
 * engine's stream for every dense step while enabled; jg_kernel_timing_read synchronises and
 * returns the average over the most recent launches (a ring of 256).  What bench.py prices the
 * roofline with when a step is more than one kernel (configs[4], the closed loop).
 * enable: 0 off, 1 every dense step, N > 1 every N-th (a pair of event records costs the stream a few
 * microseconds: a tick of three small kernels is measurably longer with every launch timed). */
int jg_kernel_timing(jg_engine* e, int enable);
int jg_kernel_timing_read(jg_engine* e, float* avg_us, uint32_t* n_launches);

/* Measurement aid (bench.py "roofline.stream_ceiling"): time a plain streaming kernel with the
 * byte profile of the dense leader tick for this engine's (G, R) — per group R 8-byte reads from
 * a rotating ack-sized buffer set larger than the Infinity Cache (non-temporal, like the ack
 * stream), two resident 8-byte columns and one 4-byte column read, one 8-byte column written —
 * and no Raft logic at all.  Same grid, workgroup size and stream as jg_step_dense_acks_device.
 * *avg_us = average launch duration over `iters` launches (HIP events).  What a launch of this
 * shape costs on the machine at hand: the practical ceiling next to the 8 TB/s spec peak. */
int jg_calibrate_stream(jg_engine* e, uint32_t iters, float* avg_us);

const char* jg_last_error(void);
uint32_t jg_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* JOSEFINE_GPU_H */
