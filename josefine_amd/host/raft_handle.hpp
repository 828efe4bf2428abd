// raft_handle.hpp — C++ host mirror of josefine's Raft driver surface over the C ABI
// (include/josefine_gpu.h).  The reference is Rust and this image has no Rust
// toolchain, so the host side above the ABI is C++ with the reference's names and
// argument meaning; the Rust adapter a maintainer would add is in INTEGRATION.md.
//
//   reference (src/raft)                              here
//   enum Command { Tick, VoteRequest{..}, .. }        josefine::Command::{Tick(), VoteRequest(..), ..}   mod.rs:160-227
//   trait Apply { fn apply(self, Command) }           josefine::RaftHandle::apply / BatchedRaft::apply     mod.rs:471-489
//   RaftHandle::{is_follower,is_candidate,is_leader}  same                                                mod.rs:437-447
//   rpc_tx: UnboundedSender<Message>                  BatchedRaft::rpc_tx  (std::function sink)           mod.rs:337-338
//   fsm_tx: UnboundedSender<Instruction>              BatchedRaft::fsm_tx  (std::function sink)           mod.rs:339-340
//   Chain's sled tree (block payloads)                josefine::BlockStore (host, key-ordered map)        chain.rs:99-104
//
// What stays on the host, exactly as in the reference: block payloads, the queued
// client requests (follower.rs:22, candidate.rs:20) and the expansion of Apply
// ranges into blocks in key order (leader.rs:93, follower.rs:204).  No state-machine
// arithmetic happens here: every decision comes out of the device engine.
#pragma once
#include <algorithm>
#include <cstdint>
#include <chrono>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/josefine_gpu.h"

#include "types.hpp"
#include "chain_store.hpp"

namespace josefine {

// Host block store of one group: what sled holds in the reference (chain.rs:99-104) - in the reference's own
// byte layout (chain_store.hpp: 8-byte big-endian keys, bincode values, the "commit" key in the same tree).
using BlockStore = formats::ChainStore;

// Command rows in the shape of jg_cmd_batch (structure of arrays): what a batched event loop queues
// between two ticks instead of one heap object per message.
struct RowQueue {
  std::vector<uint8_t> kind, flag;
  std::vector<uint32_t> group, from;
  std::vector<uint64_t> term, id, aux, blk_id, blk_next;
  size_t size() const { return kind.size(); }
  bool empty() const { return kind.empty(); }
  void clear() {
    kind.clear(), flag.clear(), group.clear(), from.clear(), term.clear(), id.clear(), aux.clear(), blk_id.clear(), blk_next.clear();
  }
  void push(uint32_t g, uint8_t k, NodeId f = 0, Term t = 0, uint64_t i = 0, uint64_t a = 0, uint8_t fl = 0) {
    kind.push_back(k), group.push_back(g), from.push_back(f), term.push_back(t), id.push_back(i), aux.push_back(a), flag.push_back(fl);
  }
  // AppendEntries{term, leader_id, blocks}: the (id, next) pairs go to the side arrays (mod.rs:196-203)
  void push_append_entries(uint32_t g, NodeId leader, Term t, const Block* blocks, size_t n) {
    push(g, JG_CMD_APPEND_ENTRIES, leader, t, blk_id.size(), n, 0);
    for (size_t k = 0; k < n; k++) blk_id.push_back(blocks[k].id), blk_next.push_back(blocks[k].next);
  }
  // the blocks (first, first + n] of a run: next = id - 1 each (what a JG_AE mailbox word stands for)
  void push_append_run(uint32_t g, NodeId leader, Term t, BlockId from_id, uint32_t n) {
    push(g, JG_CMD_APPEND_ENTRIES, leader, t, blk_id.size(), n, 0);
    for (uint32_t k = 0; k < n; k++) blk_id.push_back(from_id + 1 + k), blk_next.push_back(from_id + k);
  }
  void append(const jg_cmd_batch& b) {  // bulk: a peer's whole frame
    const uint64_t shift = blk_id.size();
    const size_t at = size();
    kind.insert(kind.end(), b.kind, b.kind + b.n), group.insert(group.end(), b.group, b.group + b.n);
    auto put = [&](auto& v, auto* src) {
      if (src) v.insert(v.end(), src, src + b.n);
      else v.resize(at + b.n, 0);
    };
    put(from, b.from), put(term, b.term), put(id, b.id), put(aux, b.aux), put(flag, b.flag);
    if (shift)
      for (size_t i = 0; i < b.n; i++)
        if (b.kind[i] == JG_CMD_APPEND_ENTRIES) id[at + i] += shift;
    if (b.n_blocks) blk_id.insert(blk_id.end(), b.blk_id, b.blk_id + b.n_blocks), blk_next.insert(blk_next.end(), b.blk_next, b.blk_next + b.n_blocks);
  }
  jg_cmd_batch view() const {
    jg_cmd_batch b{};
    b.n = kind.size();
    b.kind = kind.data(), b.group = group.data(), b.from = from.data(), b.term = term.data(), b.id = id.data(), b.aux = aux.data();
    b.flag = flag.data(), b.n_blocks = blk_id.size(), b.blk_id = blk_id.data(), b.blk_next = blk_next.data();
    return b;
  }
};

class BatchedRaft;

class RaftHandle {  // mod.rs:417-468, a view of one group
 public:
  RaftHandle(BatchedRaft* e, uint32_t g) : e_(e), g_(g) {}
  RaftHandle apply(const Command& cmd, uint64_t now_ms = 0);
  bool is_follower() const { return role() == JG_ROLE_FOLLOWER; }
  bool is_candidate() const { return role() == JG_ROLE_CANDIDATE; }
  bool is_leader() const { return role() == JG_ROLE_LEADER; }
  Term current_term() const { return read64(JG_FIELD_TERM); }
  BlockId commit() const { return read64(JG_FIELD_COMMIT); }
  BlockId head() const { return read64(JG_FIELD_HEAD); }
  uint32_t fault() const { return read8(JG_FIELD_FAULT); }
  bool has_voted() const { return read8(JG_FIELD_HAS_VOTED) != 0; }
  NodeId voted_for() const { return read32(JG_FIELD_VOTED_FOR); }

 private:
  uint8_t role() const { return read8(JG_FIELD_ROLE); }
  uint64_t read64(int f) const;
  uint32_t read32(int f) const;
  uint8_t read8(int f) const;
  BatchedRaft* e_;
  uint32_t g_;
};

class BatchedRaft {
 public:
  // sinks: everything the groups push on the two channels, in per-group order
  std::function<void(const Message&)> rpc_tx;
  std::function<void(const Instruction&)> fsm_tx;
  // batch sinks: the same two channels, a whole step at a time and in wire form - the rows as the engine
  // drains them (views of its pinned queues: no copy, no per-row object) and, for step_node, the mailbox
  // columns.  A sink that is set replaces the per-row expansion of its channel; what the rows / columns
  // stand for is in include/josefine_gpu.h.
  std::function<void(const jg_msg_row*, size_t)> msg_rows_tx;
  std::function<void(const jg_fsm_row*, size_t)> fsm_rows_tx;
  std::function<void(const jg_node_outbox&)> columns_tx;

  // RaftHandle::new for n_groups groups (mod.rs:428-435)
  // `devices`: shard the groups over these HIP devices behind this one handle (jg_config.n_devices:
  // contiguous ownership, a device may repeat) — one event loop still owns the handle, as in the
  // reference (server.rs:103-165); empty = one shard on `device`.
  // `start_vacant` (JG_CFG_START_VACANT): every slot starts vacant - a broker sizes the engine, then opens partitions.
  BatchedRaft(uint32_t n_groups, std::vector<NodeId> node_ids, int device = 0, uint64_t seed = 0,
              uint32_t flags = 0, std::vector<int> devices = {}, bool start_vacant = false)
      : stores_(n_groups), queued_(n_groups), ids_(node_ids) {
    if (start_vacant) flags |= JG_CFG_START_VACANT;
    jg_config c{};
    c.n_devices = (uint32_t)devices.size();
    for (size_t d = 0; d < devices.size() && d < JG_MAX_DEVICES; d++) c.device_ids[d] = devices[d];
    c.abi_version = JG_ABI_VERSION;
    c.n_groups = n_groups;
    c.n_replicas = (uint32_t)node_ids.size();
    for (size_t r = 0; r < node_ids.size() && r < JG_MAX_REPLICAS; r++) c.node_ids[r] = node_ids[r];
    c.device_id = device;
    c.heartbeat_timeout_ms = 100;      // config.rs:104
    c.election_timeout_min_ms = 500;   // mod.rs:318
    c.election_timeout_max_ms = 1000;  // mod.rs:319
    c.seed = seed;
    c.flags = flags;
    check(jg_engine_create(&c, &e_));
    if (!start_vacant)
      for (auto& s : stores_) s.insert(Block{0, 0, {}});  // genesis (chain.rs:139-153)
  }
  // A process that starts on the sled trees its predecessor left (Raft::<Follower>::new -> Chain::new on each,
  // follower.rs:68-95, chain.rs:117-137): stores[g] is partition g's tree (e.g. ChainStore::from_raw of what is on disk).
  // Each tree is scanned in key order - 8-byte keys are big-endian block ids, their values decoded Blocks, the "commit"
  // key read - into one jg_engine_load_chains image; the stores are adopted, so that later restarts, pumps and appends
  // write to them.  (jg_engine_load_chains is ABI v10: only callers of open() need a library that has it.)
  static std::unique_ptr<BatchedRaft> open(std::vector<NodeId> node_ids, std::vector<BlockStore> stores, uint64_t now_ms = 0,
                                           int device = 0, uint64_t seed = 0, uint32_t flags = 0, std::vector<int> devices = {},
                                           const uint8_t* self_slots = nullptr) {
    const uint32_t G = (uint32_t)stores.size();
    std::unique_ptr<BatchedRaft> r(new BatchedRaft(G, std::move(node_ids), device, seed, flags, std::move(devices)));
    if (self_slots) r->check(jg_set_self_slots(r->e_, self_slots));
    std::vector<uint64_t> off(1, 0), ids, nexts, commit(G, 0);
    std::vector<uint8_t> has(G, 0);
    for (uint32_t g = 0; g < G; g++) {
      for (const auto& kv : stores[g].raw()) {
        if (kv.first == formats::ChainStore::commit_key()) {
          commit[g] = formats::key_block_id(kv.second);
          has[g] = 1;
        } else if (kv.first.size() == 8) {
          ids.push_back(formats::key_block_id(kv.first));
          nexts.push_back(formats::decode_block(kv.second).next);
        }
      }
      off.push_back(ids.size());
    }
    jg_chain_image img{};
    img.g0 = 0, img.n = G;
    img.off = off.data(), img.blk_id = ids.data(), img.blk_next = nexts.data(), img.commit = commit.data(), img.has_commit = has.data();
    r->check(jg_engine_load_chains(r->e_, now_ms, &img));
    r->stores_ = std::move(stores);
    for (uint32_t g = 0; g < G; g++) r->stores_[g].reopen();  // Chain::new's genesis where the tree has no commit key (as restart())
    return r;
  }
  // The engine's chain trees read back out (jg_engine_read_chains, ABI v11; only callers need a library that has it): groups
  // [g0, g0 + n) as the CSR rows of a sled scan of each - what BatchedRaft::open takes, and what stores_[g] must hold.
  struct ChainRows {
    std::vector<uint64_t> off, id, next, commit;  // off [n + 1]; id / next [off[n]], ascending per group; commit [n]
    std::vector<uint8_t> has_commit, fault;       // [n]; fault >= 128: the engine's image is not the tree (no rows)
  };
  ChainRows read_chains(uint32_t g0 = 0, uint32_t n = UINT32_MAX) {
    if (n == UINT32_MAX) n = (uint32_t)stores_.size() - g0;
    ChainRows c;
    c.off.assign((size_t)n + 1, 0), c.commit.assign(n, 0), c.has_commit.assign(n, 0), c.fault.assign(n, 0);
    jg_chain_read r{};
    r.g0 = g0, r.n = n;
    r.off = c.off.data(), r.commit = c.commit.data(), r.has_commit = c.has_commit.data(), r.fault = c.fault.data();
    uint64_t rows = 0;
    int rc = jg_engine_read_chains(e_, &r, &rows);  // sized first (cap 0) ...
    if (rc == JG_ECAPACITY) {  // ... then read
      c.id.resize(rows), c.next.resize(rows);
      r.cap = rows, r.blk_id = c.id.data(), r.blk_next = c.next.data();
      rc = jg_engine_read_chains(e_, &r, &rows);
    }
    check(rc);
    return c;
  }
  // Live groups handed over to another BatchedRaft of the same node without a restart (jg_engine_export_groups /
  // jg_engine_import_groups, ABI v12; only callers need a library that has it): the engine's state image of groups
  // [g0, g0 + n) plus what the adapter keeps beside it - each group's BlockStore (the sled tree stays the same tree), its
  // queued client request tokens and the proposals behind them (a follower / candidate forwards them when it learns a
  // leader: follower.rs:190-197).  Drain this handle's rows first: what the groups already produced stays here.
  struct GroupImage {
    jg_group_image_header header{};
    std::vector<uint8_t> records;        // [n * header.record_bytes]
    std::vector<BlockStore> stores;      // [n]
    std::vector<std::deque<uint64_t>> queued;
    std::vector<std::map<uint64_t, std::vector<uint8_t>>> proposals;  // [n]: request id -> proposal
  };
  GroupImage export_groups(uint32_t g0 = 0, uint32_t n = UINT32_MAX) {
    if (n == UINT32_MAX) n = (uint32_t)stores_.size() - g0;
    GroupImage im;
    jg_group_export x{};
    x.g0 = g0, x.n = n;
    const int rc = jg_engine_export_groups(e_, &x);  // the sizing call (cap 0): the header
    if (rc != JG_ECAPACITY) check(rc);
    im.records.resize((size_t)n * x.header.record_bytes);
    x.cap_bytes = im.records.size(), x.records = im.records.data();
    check(jg_engine_export_groups(e_, &x));
    im.header = x.header;
    im.stores.assign(stores_.begin() + g0, stores_.begin() + g0 + n);
    im.queued.assign(queued_.begin() + g0, queued_.begin() + g0 + n);
    im.proposals.resize(n);
    for (auto it = pending_reqs_.lower_bound({g0, 0}); it != pending_reqs_.end() && it->first.first < g0 + n; ++it)
      im.proposals[it->first.first - g0][it->first.second] = it->second;
    return im;
  }
  // the image's groups continue at [g0, g0 + n) of this handle (its timers moved by shift_ms); their stores, queued tokens
  // and proposals are adopted (whatever these groups held here before is dropped)
  void import_groups(GroupImage im, uint32_t g0 = 0, int64_t shift_ms = 0) {
    jg_group_import y{};
    y.g0 = g0, y.shift_ms = shift_ms, y.header = im.header, y.records = im.records.data();
    check(jg_engine_import_groups(e_, &y));
    const uint32_t n = im.header.n;
    pending_reqs_.erase(pending_reqs_.lower_bound({g0, 0}), pending_reqs_.lower_bound({g0 + n, 0}));  // (what the groups held)
    for (uint32_t i = 0; i < n; i++) {
      stores_[g0 + i] = std::move(im.stores[i]);
      queued_[g0 + i] = std::move(im.queued[i]);
      for (auto& kv : im.proposals[i]) pending_reqs_[{g0 + i, kv.first}] = std::move(kv.second);
    }
  }
  // Partitions opened and closed at runtime (jg_engine_open_groups / jg_engine_close_groups / jg_engine_list_groups, ABI
  // v13; only callers need a library that has them): LeaderAndIsr creating a replica in a running broker is an open of a
  // vacant slot - what a JG_CMD_RECREATE row does, with the store reset to Chain::new's genesis; deleting one is a close,
  // which drops the slot's store, its queued request tokens and their proposals.  A vacant slot ignores every row.
  void open_groups(const std::vector<uint32_t>& groups, uint64_t now_ms, const std::vector<uint8_t>* self_slots = nullptr) {
    jg_group_set s{};
    s.n = (uint32_t)groups.size(), s.groups = groups.data(), s.self_slots = self_slots ? self_slots->data() : nullptr;
    check(jg_engine_open_groups(e_, now_ms, &s));
    for (uint32_t g : groups) {
      stores_[g] = BlockStore{};
      stores_[g].insert(Block{0, 0, {}});
      extend_failed_.erase(g);
    }
  }
  void close_groups(const std::vector<uint32_t>& groups) {
    jg_group_set s{};
    s.n = (uint32_t)groups.size(), s.groups = groups.data();
    check(jg_engine_close_groups(e_, &s));
    for (uint32_t g : groups) {
      stores_[g] = BlockStore{};
      queued_[g].clear();
      extend_failed_.erase(g);
      pending_reqs_.erase(pending_reqs_.lower_bound({g, 0}), pending_reqs_.lower_bound({g + 1, 0}));
    }
  }
  std::vector<uint32_t> list_groups(uint32_t which, uint32_t g0 = 0, uint32_t n = UINT32_MAX) {
    if (n == UINT32_MAX) n = (uint32_t)stores_.size() - g0;
    std::vector<uint32_t> out(n);
    size_t total = 0;
    check(jg_engine_list_groups(e_, which, g0, n, out.data(), out.size(), &total));
    out.resize(std::min<size_t>(total, n));
    return out;
  }
  std::vector<uint32_t> vacant_groups(uint32_t g0 = 0, uint32_t n = UINT32_MAX) { return list_groups(JG_LIST_VACANT, g0, n); }
  std::vector<uint32_t> hosted_groups(uint32_t g0 = 0, uint32_t n = UINT32_MAX) { return list_groups(JG_LIST_HOSTED, g0, n); }
  // The leadership feed and the census (jg_engine_watch_leaders / jg_engine_census, ABI v14; only callers need a library
  // that has them): the slots of [g0, g0 + n) whose leadership view - role, term, known leader, fault, vacancy - differs
  // from what this feed last reported, ascending, as their current view; at most `limit` rows, *total (if given) how many
  // differ.  The delivered slots become "seen" unless `peek`.  What a broker serves Metadata's leader_id / leader_epoch
  // from and keeps its LeaderAndIsr bookkeeping with, instead of one RaftHandle::role() round trip per partition.  ONE
  // feed per engine: the event loop that owns the handle.
  std::vector<jg_leader_row> watch_leaders(uint32_t g0 = 0, uint32_t n = UINT32_MAX, size_t limit = SIZE_MAX, bool peek = false,
                                           size_t* total = nullptr) {
    if (n == UINT32_MAX) n = (uint32_t)stores_.size() - g0;
    std::vector<jg_leader_row> out(std::min<size_t>(limit, n));
    size_t tot = 0;
    check(jg_engine_watch_leaders(e_, peek ? (uint32_t)JG_WATCH_PEEK : 0u, g0, n, out.data(), out.size(), &tot));
    out.resize(std::min<size_t>(tot, out.size()));
    if (total) *total = tot;
    return out;
  }
  jg_census census(uint32_t g0 = 0, uint32_t n = UINT32_MAX) {
    if (n == UINT32_MAX) n = (uint32_t)stores_.size() - g0;
    jg_census c{};
    check(jg_engine_census(e_, g0, n, &c));
    return c;
  }
  // The replication feed and its census (jg_engine_watch_replicas / jg_engine_replication_census, ABI v15; only callers
  // need a library that has them): the slots of [g0, g0 + n) whose in-sync set - or whether the slot leads at all - differs
  // from what this feed last reported, ascending, as their current view; at most `limit` rows, *total (if given) how many
  // differ.  A member last reported in sync stays while its lag is <= policy.leave_lag, any other joins at lag <=
  // policy.join_lag.  The delivered slots become "seen" unless `peek`.  What a broker keeps Partition.isr
  // (partition.rs:15) and Metadata's isr_nodes (metadata.rs:93) with.  ONE feed per engine.
  std::vector<jg_isr_row> watch_replicas(jg_isr_policy policy, uint32_t g0 = 0, uint32_t n = UINT32_MAX, size_t limit = SIZE_MAX,
                                         bool peek = false, size_t* total = nullptr) {
    if (n == UINT32_MAX) n = (uint32_t)stores_.size() - g0;
    std::vector<jg_isr_row> out(std::min<size_t>(limit, n));
    size_t tot = 0;
    check(jg_engine_watch_replicas(e_, peek ? (uint32_t)JG_WATCH_PEEK : 0u, &policy, g0, n, out.data(), out.size(), &tot));
    out.resize(std::min<size_t>(tot, out.size()));
    if (total) *total = tot;
    return out;
  }
  // ... under the time rule (jg_engine_watch_replicas_timed, ABI v19; only callers need a library that has it): the same
  // feed and the same shadow, but a member last reported in sync stays until it has been behind (lag > clock.caught_lag) for
  // more than clock.max_behind_ms - replica.lag.time.max.ms - of the caller's clock clock.now_ms, sampled at the calls; any
  // other joins at lag <= clock.join_lag.  Unless `peek` the clocks of every slot of the range advance, delivered or not.
  std::vector<jg_isr_row> watch_replicas_timed(jg_isr_clock clock, uint32_t g0 = 0, uint32_t n = UINT32_MAX, size_t limit = SIZE_MAX,
                                               bool peek = false, size_t* total = nullptr) {
    if (n == UINT32_MAX) n = (uint32_t)stores_.size() - g0;
    std::vector<jg_isr_row> out(std::min<size_t>(limit, n));
    size_t tot = 0;
    check(jg_engine_watch_replicas_timed(e_, peek ? (uint32_t)JG_WATCH_PEEK : 0u, &clock, g0, n, out.data(), out.size(), &tot));
    out.resize(std::min<size_t>(tot, out.size()));
    if (total) *total = tot;
    return out;
  }
  jg_repl_census replication_census(uint64_t lag_limit, uint32_t g0 = 0, uint32_t n = UINT32_MAX) {
    if (n == UINT32_MAX) n = (uint32_t)stores_.size() - g0;
    jg_repl_census c{};
    check(jg_engine_replication_census(e_, lag_limit, g0, n, &c));
    return c;
  }
  // an `isr` mask as the Vec<i32> of node ids Partition.isr holds, in member-slot order
  std::vector<int32_t> isr_nodes(uint8_t isr) const {
    std::vector<int32_t> out;
    for (size_t r = 0; r < ids_.size() && r < JG_MAX_REPLICAS; r++)
      if ((isr >> r) & 1u) out.push_back((int32_t)ids_[r]);
    return out;
  }
  // Point queries (jg_engine_lookup_groups, ABI v16; only callers need a library that has it): the state of the n listed
  // slots - any order, repeats allowed - one row per entry in the order asked: every RaftHandle getter's column of the slot
  // and its leadership view (`state`: JG_LEAD_*, `known_leader`) from one device pass, instead of one jg_read_state round
  // trip per partition and field.  With `progress`, match[i * R + r] is the progress head of member slot r of entry i (0
  // for a slot that does not lead).  What a broker answers Metadata, ListOffsets or the high watermarks of a Fetch with.
  struct GroupStates {
    std::vector<jg_group_state> rows;
    std::vector<uint64_t> match;  // [n][R] with progress, else empty
  };
  GroupStates lookup(const uint32_t* groups, size_t n, bool progress = false) {
    jg_group_set s{};
    s.n = (uint32_t)n, s.groups = groups;
    return lookup_set(s, progress);
  }
  // ... of the range [g0, g0 + n)
  GroupStates lookup(uint32_t g0, uint32_t n, bool progress = false) {
    jg_group_set s{};
    s.g0 = g0, s.n = n;
    return lookup_set(s, progress);
  }
  // The commit feed (jg_engine_watch_commits, ABI v17; only callers need a library that has it): the slots of
  // [g0, g0 + n) whose (commit, head) - with `commits_only` whose commit - differs from what this feed last delivered,
  // ascending, each with the values last delivered and the values now; at most `limit` rows, *total (if given) how many
  // differ, *backlog (if given) every differing slot of the range before this call's delivery.  The delivered slots
  // become "seen" unless `peek`.  The fsm_tx of the dense entry points, which queue no FSM rows.  ONE feed per engine.
  std::vector<jg_commit_row> watch_commits(uint32_t g0 = 0, uint32_t n = UINT32_MAX, size_t limit = SIZE_MAX, bool peek = false,
                                           bool commits_only = false, size_t* total = nullptr, jg_commit_backlog* backlog = nullptr) {
    if (n == UINT32_MAX) n = (uint32_t)stores_.size() - g0;
    std::vector<jg_commit_row> out(std::min<size_t>(limit, n));
    size_t tot = 0;
    const uint32_t flags = (peek ? (uint32_t)JG_WATCH_PEEK : 0u) | (commits_only ? (uint32_t)JG_WATCH_COMMITS_ONLY : 0u);
    check(jg_engine_watch_commits(e_, flags, g0, n, out.data(), out.size(), &tot, backlog));
    out.resize(std::min<size_t>(tot, out.size()));
    if (total) *total = tot;
    return out;
  }
  // The completion feed (jg_engine_await_open / _await_blocks / _watch_completions, ABI v22; only callers need a library
  // that has it): fsm::Driver's notifications (fsm.rs:35) as a table of waiters on the device.  open_waiters (re)sizes the
  // table (refused while waiters are outstanding; 0 frees it); await_blocks registers waiters, all or nothing;
  // watch_completions returns the waiters that are done at now_ms - applied, lost or expired: jg_done_row.state - in
  // registration order, at most `limit` rows, *total (if given) how many are done, *stats (if given) the counts before the
  // delivery and what is left.  The delivered waiters leave the table unless `peek`.
  void open_waiters(size_t capacity) { check(jg_engine_await_open(e_, capacity)); }
  void await_blocks(const std::vector<jg_await_row>& rows) { check(jg_engine_await_blocks(e_, rows.data(), rows.size())); }
  std::vector<jg_done_row> watch_completions(uint64_t now_ms = 0, size_t limit = SIZE_MAX, bool peek = false, size_t* total = nullptr,
                                             jg_await_stats* stats = nullptr) {
    size_t tot = 0;
    if (limit == SIZE_MAX) {  // everything that is done: sized by a count
      check(jg_engine_watch_completions(e_, JG_WATCH_PEEK, now_ms, nullptr, 0, &tot, nullptr));
      limit = tot;
    }
    std::vector<jg_done_row> out(limit);
    check(jg_engine_watch_completions(e_, peek ? (uint32_t)JG_WATCH_PEEK : 0u, now_ms, out.data(), out.size(), &tot, stats));
    out.resize(std::min<size_t>(tot, out.size()));
    if (total) *total = tot;
    return out;
  }
  // Withdrawing waiters (jg_engine_await_cancel, ABI v24; only callers need a library that has it): every outstanding waiter
  // whose token & mask is among `keys` (any order, repeats allowed) is marked and leaves at the next watch_completions with
  // state JG_DONE_CANCELLED, in registration order - exact tokens with the default mask, connections with the connection id
  // in the token's high bits and a mask over them, everything with keys {0} and mask 0.  Returns the waiters newly marked.
  size_t cancel_waiters(const std::vector<uint64_t>& keys, uint64_t mask = UINT64_MAX) {
    size_t marked = 0;
    check(jg_engine_await_cancel(e_, keys.data(), keys.size(), mask, &marked));
    return marked;
  }
  // One poll per tick (jg_engine_poll, ABI v18; only callers need a library that has it): the parts `want` names of
  // watch_leaders, watch_replicas, watch_commits, census and replication_census over [g0, g0 + n) in ONE call - one settle,
  // one device pass over the slots, one synchronisation - each exactly as its own call answers it, the shadows shared with
  // them.  A part not named is neither computed nor advanced.  Read the answers in the order leaders, replicas, commits: a
  // role change is known before the ranges of the commit rows are applied.  With `timed` (ABI v20) the replicas part is
  // watch_replicas_timed's under `clock` - `policy` is not read - and unless replicas_peek the clocks of every slot of the
  // range advance to clock.now_ms, whatever replicas_limit is.
  struct PollRequest {
    uint32_t want = JG_POLL_LEADERS | JG_POLL_REPLICAS | JG_POLL_COMMITS;
    uint32_t g0 = 0, n = UINT32_MAX;
    size_t leaders_limit = SIZE_MAX, replicas_limit = SIZE_MAX, commits_limit = SIZE_MAX;
    bool leaders_peek = false, replicas_peek = false, commits_peek = false;
    bool commits_only = false;
    jg_isr_policy policy{0, 0};    // JG_POLL_REPLICAS
    bool timed = false;             // JG_POLL_REPLICAS under the time rule of `clock`
    jg_isr_clock clock{0, 0, 0, 0};
    uint64_t census_lag_limit = 0;  // JG_POLL_REPL_CENSUS
  };
  struct PollResult {
    std::vector<jg_leader_row> leaders;
    std::vector<jg_isr_row> replicas;
    std::vector<jg_commit_row> commits;
    size_t leaders_total = 0, replicas_total = 0, commits_total = 0;
    jg_commit_backlog backlog{};
    jg_census census{};
    jg_repl_census repl_census{};
  };
  PollResult poll(const PollRequest& q) {
    PollResult r;
    jg_poll p{};
    p.want = q.want, p.g0 = q.g0, p.n = q.n == UINT32_MAX ? (uint32_t)stores_.size() - q.g0 : q.n;
    p.leader_flags = q.leaders_peek ? (uint32_t)JG_WATCH_PEEK : 0u;
    p.replica_flags = q.replicas_peek ? (uint32_t)JG_WATCH_PEEK : 0u;
    p.commit_flags = (q.commits_peek ? (uint32_t)JG_WATCH_PEEK : 0u) | (q.commits_only ? (uint32_t)JG_WATCH_COMMITS_ONLY : 0u);
    p.policy = q.policy, p.census_lag_limit = q.census_lag_limit;
    p.clock = q.timed ? &q.clock : nullptr;
    if (q.want & JG_POLL_LEADERS) r.leaders.resize(std::min<size_t>(q.leaders_limit, p.n));
    if (q.want & JG_POLL_REPLICAS) r.replicas.resize(std::min<size_t>(q.replicas_limit, p.n));
    if (q.want & JG_POLL_COMMITS) r.commits.resize(std::min<size_t>(q.commits_limit, p.n));
    p.leaders = r.leaders.data(), p.leaders_cap = r.leaders.size();
    p.replicas = r.replicas.data(), p.replicas_cap = r.replicas.size();
    p.commits = r.commits.data(), p.commits_cap = r.commits.size();
    p.backlog = &r.backlog, p.census = &r.census, p.repl_census = &r.repl_census;
    check(jg_engine_poll(e_, &p));
    r.leaders_total = p.leaders_total, r.replicas_total = p.replicas_total, r.commits_total = p.commits_total;
    r.leaders.resize(std::min<size_t>(r.leaders_total, r.leaders.size()));
    r.replicas.resize(std::min<size_t>(r.replicas_total, r.replicas.size()));
    r.commits.resize(std::min<size_t>(r.commits_total, r.commits.size()));
    return r;
  }
  // A poll behind a kept node step (jg_step_node_polled / jg_node_poll_view, ABI v21; only callers need a library that has
  // them): step_node_begin(now_ms, flags, true, true) with `q` attached - the poll is queued behind the step's own kernels,
  // sees the engine exactly as the step leaves it and comes home on the step's trip; node_poll() hands it out once
  // step_node_finish has served that step.  The answer is what poll(q) would have returned between that step and the next.
  void step_node_polled(uint64_t now_ms, uint32_t flags, const PollRequest& q) {
    flush_rows();
    const jg_poll p = polled_words(q);
    check(jg_step_node_polled(e_, now_ms, flags | (uint32_t)JG_NODE_ASYNC | (uint32_t)JG_NODE_KEEP, &p));
    step_blocks_.emplace_back();
    step_blocks_.back().swap(pending_blocks_);  // (as step_node_begin)
  }
  // the jg_poll of a polled step: the input fields only (q must outlive the call: its clock is pointed at)
  jg_poll polled_words(const PollRequest& q) const {
    static jg_commit_backlog wanted;  // (never written through: the pointer only says that the backlog is wanted)
    jg_poll p{};
    p.want = q.want, p.g0 = q.g0, p.n = q.n == UINT32_MAX ? (uint32_t)stores_.size() - q.g0 : q.n;
    p.leader_flags = q.leaders_peek ? (uint32_t)JG_WATCH_PEEK : 0u;
    p.replica_flags = q.replicas_peek ? (uint32_t)JG_WATCH_PEEK : 0u;
    p.commit_flags = (q.commits_peek ? (uint32_t)JG_WATCH_PEEK : 0u) | (q.commits_only ? (uint32_t)JG_WATCH_COMMITS_ONLY : 0u);
    p.policy = q.policy, p.census_lag_limit = q.census_lag_limit;
    p.clock = q.timed ? &q.clock : nullptr;
    p.leaders_cap = std::min<size_t>(q.leaders_limit, p.n), p.replicas_cap = std::min<size_t>(q.replicas_limit, p.n);
    p.commits_cap = std::min<size_t>(q.commits_limit, p.n);
    p.backlog = &wanted;
    return p;
  }
  // the poll of the kept step step_node_finish served last; *polled: that step carried one; *redone: JG_NODE_POLL_REDONE
  PollResult node_poll(bool* polled = nullptr, bool* redone = nullptr) {
    jg_node_poll v{};
    check(jg_node_poll_view(e_, &v));
    PollResult r;
    if (v.leaders_n) r.leaders.assign(v.leaders, v.leaders + v.leaders_n);
    if (v.replicas_n) r.replicas.assign(v.replicas, v.replicas + v.replicas_n);
    if (v.commits_n) r.commits.assign(v.commits, v.commits + v.commits_n);
    r.leaders_total = v.leaders_total, r.replicas_total = v.replicas_total, r.commits_total = v.commits_total;
    r.backlog = v.backlog, r.census = v.census, r.repl_census = v.repl_census;
    if (polled) *polled = v.want != 0;
    if (redone) *redone = (v.state & JG_NODE_POLL_REDONE) != 0;
    return r;
  }
  // Completions behind a kept node step (jg_step_node_awaited / jg_node_await_view, ABI v23; only callers need a library
  // that has them): the step registers `a.rows` and then watches, behind its own kernels (and behind the poll `q`, if not
  // null); node_completions() hands the answer out once step_node_finish has served that step.  The answer is what
  // await_blocks(a.rows), cancel_waiters(a.cancel_keys, a.cancel_mask) (ABI v24; no keys: no cancel) and
  // watch_completions(a.now_ms, a.limit, a.peek) would have returned between that step and the next.  The table's room is
  // checked against a bound: what outstanding steps' watches remove counts once they are finished.
  struct AwaitRequest {
    std::vector<jg_await_row> rows;
    uint64_t now_ms = 0;
    size_t limit = SIZE_MAX;
    bool peek = false, stats = false;
    std::vector<uint64_t> cancel_keys;  // withdrawn between the registration and the watch (the step's own rows too)
    uint64_t cancel_mask = UINT64_MAX;
  };
  struct Completions {
    std::vector<jg_done_row> rows;
    size_t total = 0;
    jg_await_stats stats{};  // zero unless wanted
    size_t marked = 0;       // the waiters the step's cancel newly marked
  };
  void step_node_awaited(uint64_t now_ms, uint32_t flags, const PollRequest* q, const AwaitRequest& a) {
    flush_rows();
    jg_poll p{};
    if (q) p = polled_words(*q);
    jg_node_await_request w{};
    w.rows = a.rows.data(), w.n = a.rows.size();
    w.flags = a.peek ? (uint32_t)JG_WATCH_PEEK : 0u, w.want_stats = a.stats ? 1u : 0u;
    w.now_ms = a.now_ms, w.cap = a.limit;
    if (!a.cancel_keys.empty()) w.cancel_keys = a.cancel_keys.data(), w.cancel_n = a.cancel_keys.size(), w.cancel_mask = a.cancel_mask;
    check(jg_step_node_awaited(e_, now_ms, flags | (uint32_t)JG_NODE_ASYNC | (uint32_t)JG_NODE_KEEP, q ? &p : nullptr, &w));
    step_blocks_.emplace_back();
    step_blocks_.back().swap(pending_blocks_);  // (as step_node_begin)
  }
  // the completions of the kept step step_node_finish served last; *attached: that step carried a request; *redone: JG_NODE_POLL_REDONE
  Completions node_completions(bool* attached = nullptr, bool* redone = nullptr) {
    jg_node_await v{};
    check(jg_node_await_view(e_, &v));
    Completions c;
    if (v.rows_n) c.rows.assign(v.rows, v.rows + v.rows_n);
    c.total = v.total, c.stats = v.stats, c.marked = v.marked;
    if (attached) *attached = v.attached != 0;
    if (redone) *redone = (v.state & JG_NODE_POLL_REDONE) != 0;
    return c;
  }
  // Point queries behind a kept node step (jg_step_node_looked / jg_node_lookup_view, ABI v25; only callers need a library
  // that has them): the step looks `groups` up (any order, repeats allowed, at most JG_NODE_LOOKUP_MAX), with `progress` the
  // progress heads too, behind its own kernels and behind the poll `q` and the completion request `a` (null: not attached);
  // node_lookup() hands the answer out once step_node_finish has served that step.  The answer is what lookup(groups, n,
  // progress) would have returned between that step and the next.  The list is copied by the call.
  void step_node_looked(uint64_t now_ms, uint32_t flags, const PollRequest* q, const AwaitRequest* a, const uint32_t* groups, size_t n,
                        bool progress = false) {
    flush_rows();
    static const uint32_t none = 0;  // (an empty list is still a list)
    jg_poll p{};
    if (q) p = polled_words(*q);
    jg_node_await_request w{};
    if (a) {
      w.rows = a->rows.data(), w.n = a->rows.size();
      w.flags = a->peek ? (uint32_t)JG_WATCH_PEEK : 0u, w.want_stats = a->stats ? 1u : 0u;
      w.now_ms = a->now_ms, w.cap = a->limit;
      if (!a->cancel_keys.empty()) w.cancel_keys = a->cancel_keys.data(), w.cancel_n = a->cancel_keys.size(), w.cancel_mask = a->cancel_mask;
    }
    if (n > JG_NODE_LOOKUP_MAX) throw EngineError(JG_EINVAL, "step_node_looked: more than JG_NODE_LOOKUP_MAX entries");
    jg_group_set s{};
    s.n = (uint32_t)n, s.groups = n ? groups : &none, s.flags = progress ? (uint32_t)JG_LOOKUP_PROGRESS : 0u;
    check(jg_step_node_looked(e_, now_ms, flags | (uint32_t)JG_NODE_ASYNC | (uint32_t)JG_NODE_KEEP, q ? &p : nullptr, a ? &w : nullptr, &s));
    step_blocks_.emplace_back();
    step_blocks_.back().swap(pending_blocks_);  // (as step_node_begin)
  }
  // the lookup of the kept step step_node_finish served last; *attached: that step carried one; *redone: JG_NODE_POLL_REDONE
  GroupStates node_lookup(bool* attached = nullptr, bool* redone = nullptr) {
    jg_node_lookup v{};
    check(jg_node_lookup_view(e_, &v));
    GroupStates out;
    if (v.n) out.rows.assign(v.rows, v.rows + v.n);
    if (v.n && v.match) out.match.assign(v.match, v.match + v.n * ids_.size());
    if (attached) *attached = v.attached != 0;
    if (redone) *redone = (v.state & JG_NODE_POLL_REDONE) != 0;
    return out;
  }
  // Partitions opened and closed behind a kept node step (jg_step_node_hosted / jg_node_hosting_view, ABI v26; only callers
  // need a library that has them): behind everything else of the step - its own kernels, the poll `q`, the completion
  // request `a`, the lookup (`looked`: of `groups`, as step_node_looked) - the engine becomes what close_groups(h.close) and
  // then open_groups(h.open, now_ms, h.self_slots) make of it; each list strictly ascending, at most JG_NODE_HOSTING_MAX
  // entries.  A set the synchronous call would refuse for a slot's state writes nothing and does not affect the other.
  // node_hosting() hands the verdict out once step_node_finish has served that step; step_node_finish itself applies to this
  // mirror what the sets wrote, behind the step's own blocks - the stores of closed and opened partitions start over, a
  // closed partition's queued tokens and proposals are dropped.  The lists are copied by the call.
  struct Hosting {
    bool has_close = false, has_open = false, has_self = false;
    std::vector<uint32_t> close, open;
    std::vector<uint8_t> self_slots;  // has_self: one own slot per entry of `open`
  };
  struct HostingVerdict {
    bool attached = false, redone = false, close_refused = false, open_refused = false;
    uint32_t closed = 0, opened = 0;  // the slots each set wrote: its length, or 0
  };
  void step_node_hosted(uint64_t now_ms, uint32_t flags, const PollRequest* q, const AwaitRequest* a, bool looked, const uint32_t* groups, size_t n,
                        bool progress, const Hosting& h) {
    flush_rows();
    static const uint32_t none = 0;  // (an empty list is still a list)
    jg_poll p{};
    if (q) p = polled_words(*q);
    jg_node_await_request w{};
    if (a) {
      w.rows = a->rows.data(), w.n = a->rows.size();
      w.flags = a->peek ? (uint32_t)JG_WATCH_PEEK : 0u, w.want_stats = a->stats ? 1u : 0u;
      w.now_ms = a->now_ms, w.cap = a->limit;
      if (!a->cancel_keys.empty()) w.cancel_keys = a->cancel_keys.data(), w.cancel_n = a->cancel_keys.size(), w.cancel_mask = a->cancel_mask;
    }
    if (looked && n > JG_NODE_LOOKUP_MAX) throw EngineError(JG_EINVAL, "step_node_hosted: more than JG_NODE_LOOKUP_MAX entries");
    if (h.close.size() > JG_NODE_HOSTING_MAX || h.open.size() > JG_NODE_HOSTING_MAX) throw EngineError(JG_EINVAL, "step_node_hosted: more than JG_NODE_HOSTING_MAX entries");
    if (h.has_self && h.self_slots.size() != h.open.size()) throw EngineError(JG_EINVAL, "step_node_hosted: one own slot per opened slot");
    jg_group_set s{}, sc{}, so{};
    s.n = (uint32_t)n, s.groups = n ? groups : &none, s.flags = progress ? (uint32_t)JG_LOOKUP_PROGRESS : 0u;
    sc.n = (uint32_t)h.close.size(), sc.groups = sc.n ? h.close.data() : &none;
    so.n = (uint32_t)h.open.size(), so.groups = so.n ? h.open.data() : &none;
    so.self_slots = h.has_self && so.n ? h.self_slots.data() : nullptr;
    jg_node_hosting_request r{};
    r.close = h.has_close ? &sc : nullptr, r.open = h.has_open ? &so : nullptr;
    const size_t ordinal = steps_finished_ + step_blocks_.size();
    check(jg_step_node_hosted(e_, now_ms, flags | (uint32_t)JG_NODE_ASYNC | (uint32_t)JG_NODE_KEEP, q ? &p : nullptr, a ? &w : nullptr,
                              looked ? &s : nullptr, &r));
    step_blocks_.emplace_back();
    step_blocks_.back().swap(pending_blocks_);  // (as step_node_begin)
    hosted_.push_back({ordinal, h});
    if (!follow_hosting_)  // (set here, so that only a program that begins hosted steps names jg_node_hosting_view)
      follow_hosting_ = [this]() {
        jg_node_hosting v{};
        check(jg_node_hosting_view(e_, &v));
        const Hosting h = std::move(hosted_.front().second);
        hosted_.pop_front();
        if (v.closed)
          for (uint32_t g : h.close) {
            stores_[g] = BlockStore{};
            queued_[g].clear();
            extend_failed_.erase(g);
            pending_reqs_.erase(pending_reqs_.lower_bound({g, 0}), pending_reqs_.lower_bound({g + 1, 0}));
          }
        if (v.opened)
          for (uint32_t g : h.open) {
            stores_[g] = BlockStore{};
            stores_[g].insert(Block{0, 0, {}});
            extend_failed_.erase(g);
          }
      };
  }
  // the verdict of the kept step step_node_finish served last (attached == false: it carried no hosting request)
  HostingVerdict node_hosting() {
    jg_node_hosting v{};
    check(jg_node_hosting_view(e_, &v));
    HostingVerdict out;
    out.attached = v.attached != 0, out.redone = (v.state & JG_NODE_POLL_REDONE) != 0;
    out.close_refused = (v.state & JG_NODE_HOSTING_CLOSE_REFUSED) != 0, out.open_refused = (v.state & JG_NODE_HOSTING_OPEN_REFUSED) != 0;
    out.closed = v.closed, out.opened = v.opened;
    return out;
  }
  // commit rows as the FSM rows a dense step does not queue: every row that is COMMITTED and not REWOUND becomes
  // JG_FSM_APPLY_LEADER (where LEADS: keys (a, b]) or JG_FSM_APPLY_FOLLOWER (keys [a, b)) {a = commit_from, b = commit}; a
  // rewound row has no range - the consumer resynchronises its store from the row's commit / head
  static std::vector<jg_fsm_row> as_fsm_rows(const std::vector<jg_commit_row>& rows) {
    std::vector<jg_fsm_row> out;
    for (const jg_commit_row& r : rows) {
      if (!(r.state & JG_CMT_COMMITTED) || (r.state & JG_CMT_REWOUND)) continue;
      jg_fsm_row x{};
      x.group = r.group;
      x.kind = (r.state & JG_CMT_LEADS) ? (uint8_t)JG_FSM_APPLY_LEADER : (uint8_t)JG_FSM_APPLY_FOLLOWER;
      x.a = r.commit_from, x.b = r.commit;
      out.push_back(x);
    }
    return out;
  }
  ~BatchedRaft() { jg_engine_destroy(e_); }
  BatchedRaft(const BatchedRaft&) = delete;
  BatchedRaft& operator=(const BatchedRaft&) = delete;

  RaftHandle handle(uint32_t g) { return RaftHandle(this, g); }
  const BlockStore& store(uint32_t g) const { return stores_[g]; }
  jg_engine* raw() { return e_; }

  // Apply::apply for one group: submit, step, forward the outputs to the sinks.
  RaftHandle apply(uint32_t g, const Command& cmd, uint64_t now_ms = 0) {
    submit(g, cmd);
    step(now_ms);
    return RaftHandle(this, g);
  }

  void submit(uint32_t g, const Command& cmd) {
    kind_.push_back(cmd.kind);
    group_.push_back(g);
    from_.push_back(cmd.from);
    term_.push_back(cmd.term);
    flag_.push_back(cmd.flag ? 1 : 0);
    if (cmd.kind == JG_CMD_APPEND_ENTRIES) {
      id_.push_back(blk_id_.size());
      aux_.push_back(cmd.blocks.size());
      for (const Block& b : cmd.blocks) {
        blk_id_.push_back(b.id);
        blk_next_.push_back(b.next);
        pending_blocks_.push_back({g, b});  // payload goes to the host store on extend
      }
    } else {
      id_.push_back(cmd.id);
      aux_.push_back(cmd.aux);
    }
    if (cmd.kind == JG_CMD_CLIENT_REQUEST) pending_reqs_[{g, cmd.id}] = cmd.proposal;
  }

  void step(uint64_t now_ms) {
    flush_rows();
    check(jg_step(e_, now_ms));
    after_step();
  }

  // a whole frame of rows at once (no payloads: block data and proposals travel through submit())
  void submit_rows(const jg_cmd_batch& b) {
    flush_rows();
    check(jg_submit(e_, &b));
  }
  // What event_loop does between two ticks, for every partition at once (jg_step_node): the queued rows
  // - the steady-state vocabulary through the dense kernels, anything else through the general state
  // machine - then Command::Tick (JG_NODE_TICK).  The Tick's messages and the followers' answers leave as
  // mailbox columns (columns_tx, or expanded into Messages for rpc_tx); `answers_to[g]`: the NodeId a
  // follower's dense answers are addressed to (the sender of the partition's Heartbeat / AppendEntries).
  void step_node(uint64_t now_ms, uint32_t flags, const std::vector<NodeId>* answers_to = nullptr) {
    step_node_begin(now_ms, flags);
    step_node_finish(answers_to);
  }
  // The node step in two halves, so that ONE loop overlaps with itself: begin() returns as soon as the rows are on the
  // device and classified (the engine's pinned input columns are free again) with the dense halves, the fsm build and the
  // downloads of the outputs still running; the caller decodes the NEXT tick's traffic meanwhile and calls finish() -
  // which waits for the outputs, feeds fsm_tx / rpc_tx / the column sink - right before the next begin().
  // keep (JG_NODE_KEEP, with async): TWO steps in flight - begin() may be called again before the step before has been
  // finished; finish() then serves the OLDER one (its outbox, its rows), while the device runs the newer.
  void step_node_begin(uint64_t now_ms, uint32_t flags, bool async = false, bool keep = false) {
    flush_rows();
    // async: no synchronisation at all inside the call (JG_NODE_ASYNC) - the engine settles the step (its general path, if
    // it has one) when step_node_finish asks for the outbox
    check(jg_step_node(e_, now_ms, flags | (async ? (uint32_t)JG_NODE_ASYNC : 0u) | (keep ? (uint32_t)JG_NODE_KEEP : 0u)));
    step_blocks_.emplace_back();
    step_blocks_.back().swap(pending_blocks_);  // (the payloads of THIS step's AppendEntries rows: stored when it is finished)
  }
  double ms_waited_for_outputs = 0;  // inside jg_node_outbox_view, summed over the steps finished so far (a loop's own accounting)
  bool node_step_open() const { return !step_blocks_.empty(); }
  size_t replicas() const { return ids_.size(); }
  size_t node_steps_open() const { return step_blocks_.size(); }
  void step_node_finish(const std::vector<NodeId>* answers_to = nullptr) {
    if (step_blocks_.empty()) return;
    jg_node_outbox o{};
    const auto w0 = std::chrono::steady_clock::now();
    check(jg_node_outbox_view(e_, &o));  // (the oldest open step's)
    ms_waited_for_outputs += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    last_outbox_ = o;
    // (what was noted since begin() - an AppendEntries submitted meanwhile - belongs to a later step: it waits for that one)
    std::vector<std::pair<uint32_t, Block>> later = std::move(step_blocks_.front());
    step_blocks_.pop_front();
    steps_finished_++;
    later.swap(pending_blocks_);
    after_step();  // (stores this step's blocks and leaves none pending)
    if (!hosted_.empty() && hosted_.front().first + 1 == steps_finished_) follow_hosting_();  // (a hosted step: what it closed and opened, behind its own blocks)
    pending_blocks_.insert(pending_blocks_.begin(), std::make_move_iterator(later.begin()), std::make_move_iterator(later.end()));
    if (columns_tx) columns_tx(o);
    else if (rpc_tx) expand_columns(o, answers_to);
  }
  // zero-copy inbound rows: the engine's own pinned columns, filled in place by the transport's decoder
  jg_cmd_cols reserve_rows(size_t n, size_t n_blocks = 0) {
    flush_rows();
    jg_cmd_cols c{};
    check(jg_submit_reserve(e_, n, n_blocks, &c));
    return c;
  }
  void commit_rows(size_t n, size_t n_blocks, uint32_t optional_columns) { check(jg_submit_commit(e_, n, n_blocks, optional_columns)); }
  // column inbound (jg_node_inbox_columns): where member slot `slot`'s answer words (and HeartbeatResponse.commit
  // values) for the next step_node are to be written, in the engine's pinned memory
  void inbox_columns(uint32_t slot, uint64_t** answer, uint64_t** hb_commit) { check(jg_node_inbox_columns(e_, slot, answer, hb_commit)); }
  const jg_node_outbox& last_outbox() const { return last_outbox_; }
  // payload mirrors for rows that were queued in bulk (submit_rows): a ClientRequest's proposal, a block's data
  void note_proposal(uint32_t g, uint64_t request_id, std::vector<uint8_t> proposal) { pending_reqs_[{g, request_id}] = std::move(proposal); }
  void note_block(uint32_t g, const Block& b) { pending_blocks_.push_back({g, b}); }
  void store_block(uint32_t g, const Block& b) { stores_[g].insert(b); }
  // process restart of partition g's replica: the sled tree is re-opened from its bytes (ChainStore::from_raw)
  // and the engine restarts the instance on its own image of it (JG_CMD_RESTART = Raft::new + Chain::new on the
  // persisted tree, follower.rs:68-95, chain.rs:117-137); returns what Chain::new finds in the re-opened tree
  formats::ChainStore::Reopened restart(uint32_t g, uint64_t now_ms = 0) {
    stores_[g] = formats::ChainStore::from_raw(stores_[g].raw());
    extend_failed_.erase(g);
    const formats::ChainStore::Reopened r = stores_[g].reopen();
    queued_[g].clear();
    Command c;
    c.kind = JG_CMD_RESTART;
    submit(g, c);
    step(now_ms);
    return r;
  }
  // the replica of a partition that was RE-CREATED: an empty data directory (JG_CMD_RECREATE) - the host's block
  // store of the group starts over with genesis (chain.rs:139-153), like the engine's image of it
  void recreate(uint32_t g, uint64_t now_ms = 0) {
    stores_[g] = BlockStore{};
    stores_[g].insert(Block{0, 0, {}});
    extend_failed_.erase(g);
    queued_[g].clear();
    Command c;
    c.kind = JG_CMD_RECREATE;
    submit(g, c);
    step(now_ms);
  }
  NodeId self_id(uint32_t g) {
    uint8_t s = 0;
    check(jg_read_state(e_, JG_FIELD_SELF_SLOT, 0, &s, g, 1));
    return ids_[s];
  }

 private:
  friend class RaftHandle;
  void check(int rc) {
    if (rc != JG_OK) throw EngineError(rc, jg_last_error());
  }
  GroupStates lookup_set(jg_group_set& s, bool progress) {
    GroupStates out;
    out.rows.resize(s.n);
    if (progress) out.match.resize((size_t)s.n * ids_.size()), s.flags |= JG_LOOKUP_PROGRESS;
    // (an empty vector's data() may be null: JG_LOOKUP_PROGRESS wants a pointer even for no entries)
    uint64_t none = 0;
    check(jg_engine_lookup_groups(e_, &s, out.rows.data(), progress ? (out.match.empty() ? &none : out.match.data()) : nullptr));
    return out;
  }
  void flush_rows() {
    if (kind_.empty()) return;
    jg_cmd_batch b{};
    b.n = kind_.size();
    b.kind = kind_.data(), b.group = group_.data(), b.from = from_.data(), b.term = term_.data();
    b.id = id_.data(), b.aux = aux_.data(), b.flag = flag_.data();
    b.n_blocks = blk_id_.size(), b.blk_id = blk_id_.data(), b.blk_next = blk_next_.data();
    check(jg_submit(e_, &b));
    kind_.clear(), group_.clear(), from_.clear(), term_.clear(), id_.clear(), aux_.clear(), flag_.clear();
    blk_id_.clear(), blk_next_.clear();
  }
  void after_step() {
    // followers store the payloads of the blocks they were sent exactly as Chain::extend does (chain.rs:178-192): a
    // block whose parent is missing returns Err BEFORE db.insert, the event loop of that partition ends there
    // (server.rs:125-159 propagates with `?`) and nothing behind it is stored; a partition whose process was gone
    // before the AppendEntries (or that died of something else on the way: the stale-leader assert of
    // follower.rs:147-154 comes before the extends) stores nothing - the tree must stay byte for byte what sled holds.
    if (!pending_blocks_.empty()) {
      uint32_t lo = pending_blocks_.front().first, hi = lo;
      for (auto& pb : pending_blocks_) lo = std::min(lo, pb.first), hi = std::max(hi, pb.first);
      std::vector<uint8_t> fault(hi - lo + 1);
      check(jg_read_state(e_, JG_FIELD_FAULT, 0, fault.data(), lo, hi - lo + 1));
      for (auto& pb : pending_blocks_) {
        const uint32_t g = pb.first;
        uint8_t& f = fault[g - lo];
        if (f && (f != JG_FAULT_EXTEND_MISSING_PARENT || extend_failed_.count(g))) continue;
        if (f == JG_FAULT_EXTEND_MISSING_PARENT && !stores_[g].has(pb.second.next)) {
          extend_failed_.insert(g);  // the failing block: dropped, and everything of this partition behind it
          continue;
        }
        stores_[g].insert(pb.second);
      }
    }
    pending_blocks_.clear();
    pump();
  }
  // the mailbox columns as the Messages they stand for (include/josefine_gpu.h, "dense node tick")
  void expand_columns(const jg_node_outbox& o, const std::vector<NodeId>* answers_to) {
    const uint32_t G = (uint32_t)stores_.size(), R = (uint32_t)ids_.size();
    if (o.beat)
      for (uint32_t g = 0; g < G; g++) {
        jg_msg_row r{};
        r.group = g, r.term = o.beat[g].term;
        bool have_from = false;
        auto from = [&] {
          if (!have_from) r.from = self_id(g), have_from = true;
        };
        if (o.beat[g].hb_commit != JG_NO_ACK) {  // Heartbeat{term, commit, leader_id} to everybody (leader.rs:44-51)
          from();
          r.kind = JG_CMD_HEARTBEAT, r.to_kind = JG_TO_PEERS, r.to_id = 0, r.id = o.beat[g].hb_commit, r.aux = 0;
          emit(r, r.id);
        }
        // (JG_NODE_COMMON_AE: one word for every addressee unless the partition's words differ)
        const bool common = o.aec && o.aec[g] != JG_AEC_INDIVIDUAL;
        if (common && o.aec[g] == JG_NO_ACK) continue;
        if (common) from();
        for (uint32_t q = 0; q < R; q++) {  // AppendEntries per follower, ascending slot (leader.rs:124-174)
          if (common && ids_[q] == r.from) continue;
          const uint64_t w = common ? o.aec[g] : o.ae[(size_t)q * G + g];
          if (w == JG_NO_ACK) continue;
          from();
          r.kind = JG_CMD_APPEND_ENTRIES, r.to_kind = JG_TO_PEER, r.to_id = ids_[q], r.id = w >> 8, r.aux = w & 0xffu;
          emit(r, r.id);
        }
      }
    if (o.answer)
      for (uint32_t g = 0; g < G; g++) {
        const uint64_t w = o.answer[g];
        if (w == JG_NO_ACK) continue;
        jg_msg_row r{};
        r.group = g, r.from = self_id(g), r.to_kind = JG_TO_PEER, r.to_id = answers_to ? (*answers_to)[g] : 0;
        if ((w & 0xffu) != JG_HB_NONE) {  // HeartbeatResponse first: the Heartbeat was applied first (follower.rs:209-215)
          r.kind = JG_CMD_HEARTBEAT_RESPONSE, r.flag = (uint8_t)(w & 0xffu), r.term = 0, r.id = o.hb_commit[g], r.aux = 0;
          emit(r, r.id);
        }
        if ((w >> 8) != JG_MAILBOX_NONE) {  // AppendResponse{node_id, head, success} (follower.rs:163-172); its `term` is
          r.kind = JG_CMD_APPEND_RESPONSE, r.flag = 1, r.term = 0, r.id = w >> 8, r.aux = 0;  // not on the dense wire: no
          emit(r, r.id);                                                                    // leader reads it (leader.rs:211-219)
        }
      }
  }

  void pump() {
    size_t n = 0;
    if (fsm_rows_tx && msg_rows_tx) {  // batch sinks on both channels: the engine's pinned queues as they are
      const jg_fsm_row* fv = nullptr;
      check(jg_drain_applies_view(e_, &fv, &n));
      if (n) fsm_rows_tx(fv, n);
      const jg_msg_row* mv = nullptr;
      check(jg_drain_messages_view(e_, &mv, &n));
      if (n) msg_rows_tx(mv, n);
      return;
    }
    check(jg_drain_applies(e_, nullptr, 0, &n));
    std::vector<jg_fsm_row> fr(n);
    if (n) check(jg_drain_applies(e_, fr.data(), n, &n));
    if (fsm_rows_tx) {
      if (n) fsm_rows_tx(fr.data(), n);
      fr.clear();
    }
    auto deliver = [&](const jg_fsm_row& r) {
      BlockStore& st = stores_[r.group];
      if (r.kind == JG_FSM_NOTIFY) {
        // leader append (leader.rs:177-188): the block now exists with the request's payload
        Block b{r.a, r.a ? st.prev_key(r.a) : 0, {}};
        auto it = pending_reqs_.find({r.group, r.b});
        if (it != pending_reqs_.end()) {
          b.data = it->second;
          pending_reqs_.erase(it);
        }
        st.insert(b);
        if (fsm_tx) {
          Instruction ins;
          ins.kind = Instruction::Notify, ins.group = r.group, ins.request_id = r.b, ins.block_id = r.a;
          fsm_tx(ins);
        }
      } else {
        // range(a..=b).skip(1) for the leader (leader.rs:93), range(a..b) for a follower
        // (follower.rs:204): by key order over what is stored, not by parent pointers.
        st.set_commit(r.b);  // chain.commit(id) persists the "commit" key first (chain.rs:195-205)
        const BlockId hi = r.b;
        const std::vector<Block> blocks = st.range(r.a, &hi, r.kind == JG_FSM_APPLY_LEADER);
        bool skip = r.kind == JG_FSM_APPLY_LEADER;
        for (const Block& blk : blocks) {
          if (skip) {
            skip = false;
            continue;
          }
          if (fsm_tx) {
            Instruction ins;
            ins.kind = Instruction::Apply, ins.group = r.group, ins.block = blk;
            fsm_tx(ins);
          }
        }
      }
    };
    for (const jg_fsm_row& r : fr) {
      if (r.kind != JG_FSM_LEADER_STEP) {
        deliver(r);
        continue;
      }
      // JG_NODE_FSM_FUSED: a leader's step as one row - Apply {c0, c1}, Notify {a, b}, Apply {c1, c2} (josefine_gpu.h)
      const uint64_t c0 = r.a - r.pad[0], c1 = r.a - r.pad[1], c2 = r.a - r.pad[2];
      jg_fsm_row x{};
      x.group = r.group;
      if (c1 != c0) x.kind = JG_FSM_APPLY_LEADER, x.a = c0, x.b = c1, deliver(x);
      x.kind = JG_FSM_NOTIFY, x.a = r.a, x.b = r.b, deliver(x);
      if (c2 != c1) x.kind = JG_FSM_APPLY_LEADER, x.a = c1, x.b = c2, deliver(x);
    }
    check(jg_drain_messages(e_, nullptr, 0, &n));
    std::vector<jg_msg_row> mr(n);
    if (n) check(jg_drain_messages(e_, mr.data(), n, &n));
    if (msg_rows_tx) {
      if (n) msg_rows_tx(mr.data(), n);
      mr.clear();
    }
    for (const jg_msg_row& r : mr) {
      std::deque<uint64_t>& q = queued_[r.group];
      if (r.kind == JG_CMD_CLIENT_REQUEST && r.to_kind == JG_TO_QUEUE) {
        if (r.flag == JG_QUEUE_DROP) q.clear();  // follower.rs:295 / candidate.rs:216-238
        else q.push_back(r.id);                  // follower.rs:268, candidate.rs:191
        continue;
      }
      if (r.kind == JG_CMD_CLIENT_REQUEST && r.flag == JG_QUEUE_FLUSH) {  // follower.rs:190-197
        for (uint64_t tok : q) emit(r, tok);
        q.clear();
        continue;
      }
      emit(r, r.id);
    }
  }
  void emit(const jg_msg_row& r, uint64_t id) {
    if (!rpc_tx) return;
    Message m;
    m.group = r.group;
    m.from = Address{JG_TO_PEER, r.from};
    m.to = Address{r.to_kind, r.to_id};
    m.command.kind = r.kind;
    m.command.from = r.from;
    m.command.term = r.term;
    m.command.id = id;
    m.command.aux = r.aux;
    m.command.flag = r.flag != 0 && r.kind != JG_CMD_CLIENT_REQUEST;
    if (r.kind == JG_CMD_APPEND_ENTRIES) {  // leader.rs:124-174: range(id..).skip(1).take(aux)
      // (the engine has counted the blocks: the iterator is never pulled past them into the "commit" key, Q9)
      const std::vector<Block> blocks = stores_[r.group].range(r.id, nullptr, false, (size_t)r.aux + 1);
      for (size_t k = 1; k < blocks.size(); k++) m.command.blocks.push_back(blocks[k]);
    }
    if (r.kind == JG_CMD_CLIENT_REQUEST) {
      auto it = pending_reqs_.find({r.group, id});
      if (it != pending_reqs_.end()) m.command.proposal = it->second;
    }
    rpc_tx(m);
  }
  jg_engine* e_ = nullptr;
  jg_node_outbox last_outbox_{};
  std::vector<BlockStore> stores_;
  std::vector<std::deque<uint64_t>> queued_;
  std::vector<NodeId> ids_;
  std::vector<uint8_t> kind_, flag_;
  std::vector<uint32_t> group_, from_;
  std::vector<uint64_t> term_, id_, aux_, blk_id_, blk_next_;
  std::vector<std::pair<uint32_t, Block>> pending_blocks_;
  std::deque<std::vector<std::pair<uint32_t, Block>>> step_blocks_;  // one entry per node step begun and not finished (oldest first)
  size_t steps_finished_ = 0;                           // node steps step_node_finish has served
  std::deque<std::pair<size_t, Hosting>> hosted_;       // step_node_hosted: (which step, its sets) until step_node_finish has served that step
  std::function<void()> follow_hosting_;                // ... and what the mirror owes the oldest of them then
  std::set<uint32_t> extend_failed_;  // partitions whose process died in Chain::extend (until their restart)
  std::map<std::pair<uint32_t, uint64_t>, std::vector<uint8_t>> pending_reqs_;
};

// ---- dense node tick over device-resident mailboxes -------------------------------------------
// The steady-state loop of a batched event loop (server.rs:103-165 for many partitions): per
// TICK one leader half on the node that leads and one follower half on every other node, the
// messages being columns in HBM (include/josefine_gpu.h "dense node tick").  `DenseCluster`
// owns the mailbox columns of one leader node and its followers when all of them live in this
// process (one engine per node; e.g. the 3 brokers of examples/multi-node in one runtime) and
// chains the engines' streams with jg_stream_wait — no host synchronisation per round.
class DenseCluster {
 public:
  // nodes[r] hosts replica slot r of every group; nodes[lead] leads them
  DenseCluster(std::vector<jg_engine*> nodes, uint32_t n_groups, uint32_t lead, NodeId lead_id)
      : nodes_(std::move(nodes)), G_(n_groups), R_((uint32_t)nodes_.size()), lead_(lead), lead_id_(lead_id) {
    jg_engine* L = nodes_[lead_];
    answers_ = (uint64_t*)alloc(L, 8ull * R_ * G_);  // the leader's inbox: one answer word per slot and group
    hbr_commit_ = (uint64_t*)alloc(L, 8ull * R_ * G_);
    o_beat_ = (jg_leader_beat*)alloc(L, sizeof(jg_leader_beat) * (size_t)G_);
    o_ae_ = (uint64_t*)alloc(L, 8ull * R_ * G_);
    std::vector<uint64_t> a((size_t)R_ * G_, JG_NO_ACK);  // nothing from anybody; own slot: zero appends
    for (uint32_t g = 0; g < G_; g++) a[(size_t)lead_ * G_ + g] = JG_ANSWER(0, JG_HB_NONE);
    check(jg_device_upload(L, answers_, a.data(), a.size() * 8));
    std::fill(a.begin(), a.end(), JG_NO_ACK);  // (the lead node's own row of the AppendEntries block is never written: jg_leader_outbox)
    check(jg_device_upload(L, o_ae_, a.data(), a.size() * 8));
  }
  ~DenseCluster() {
    for (void* p : bufs_) (void)jg_device_free(nodes_[lead_], p);
  }
  // number of ClientRequests every group appends in the next round (leader.rs:177-197)
  void set_appends(const std::vector<uint64_t>& n) {
    std::vector<uint64_t> w(G_);  // the own slot's answer words
    for (uint32_t g = 0; g < G_; g++) w[g] = JG_ANSWER(n[g], JG_HB_NONE);
    check(jg_device_upload(nodes_[lead_], answers_ + (size_t)lead_ * G_, w.data(), (size_t)G_ * 8));
  }
  // one protocol round at logical time now_ms
  void round(uint64_t now_ms) {
    jg_engine* L = nodes_[lead_];
    for (uint32_t r = 0; r < R_; r++)
      if (r != lead_) check(jg_stream_wait(L, nodes_[r]));  // last round's answers are in
    jg_leader_inbox in{answers_, hbr_commit_};
    jg_leader_outbox out{o_beat_, o_ae_};
    check(jg_step_dense_leader(L, now_ms, &in, &out));
    for (uint32_t r = 0; r < R_; r++) {
      if (r == lead_) continue;
      check(jg_stream_wait(nodes_[r], L));
      jg_follower_inbox fi{};
      fi.leader = nullptr, fi.leader_id = lead_id_;
      fi.beat = o_beat_, fi.ae = o_ae_ + (size_t)r * G_;
      jg_follower_outbox fo{answers_ + (size_t)r * G_, hbr_commit_ + (size_t)r * G_};
      check(jg_step_dense_follower(nodes_[r], now_ms, &fi, &fo, 1));
    }
  }
  void sync() {
    for (jg_engine* e : nodes_) check(jg_sync(e));
  }

 private:
  static void check(int rc) {
    if (rc != JG_OK) throw EngineError(rc, jg_last_error());
  }
  void* alloc(jg_engine* e, size_t bytes) {
    void* p = nullptr;
    check(jg_device_alloc(e, bytes, &p));
    bufs_.push_back(p);
    return p;
  }
  std::vector<jg_engine*> nodes_;
  uint32_t G_, R_, lead_;
  NodeId lead_id_;
  uint64_t *answers_, *hbr_commit_, *o_ae_;
  jg_leader_beat* o_beat_;
  std::vector<void*> bufs_;
};

// The same closed loop driven from inside the library (jg_dense_cluster_*: the round replayed as a
// hipGraph), and - round_routed - with the library's device-side transport for everything outside the
// mailbox vocabulary: the votes of an election travel between the nodes' engines without a host in
// between (the in-process stand-in for rpc_tx -> tcp.rs -> the peer's event_loop, server.rs:127-137).
class LibraryCluster {
 public:
  LibraryCluster(const std::vector<jg_engine*>& nodes, uint32_t lead) : R_((uint32_t)nodes.size()) {
    check(jg_dense_cluster_create(nodes.data(), R_, lead, &c_));
  }
  ~LibraryCluster() { jg_dense_cluster_destroy(c_); }
  LibraryCluster(const LibraryCluster&) = delete;
  LibraryCluster& operator=(const LibraryCluster&) = delete;
  void set_appends(uint64_t per_group_and_round) { check(jg_dense_cluster_set_appends(c_, per_group_and_round, nullptr)); }
  void rounds(uint64_t now_ms, uint64_t dt_ms, uint32_t n) { check(jg_dense_cluster_rounds(c_, now_ms, dt_ms, n)); }
  // `inject`: per node a device batch (jg_step_device_rows' form) or n == 0; empty = nothing for anybody
  jg_route_stats round_routed(uint64_t now_ms, const std::vector<jg_cmd_batch>& inject = {}) {
    jg_route_stats st{};
    check(jg_dense_cluster_round_routed(c_, now_ms, inject.empty() ? nullptr : inject.data(), &st));
    return st;
  }

 private:
  static void check(int rc) {
    if (rc != JG_OK) throw EngineError(rc, jg_last_error());
  }
  uint32_t R_;
  jg_dense_cluster* c_ = nullptr;
};

// ---- fsm::Driver and server::event_loop for many partitions ---------------------------------------
// The two tasks on either side of Raft<T> in a josefine process, batched over every partition the
// process hosts.  Logical time: `run_until(now_ms)` plays the
// interval timer of server.rs:25,113 (one Command::Tick per partition every 100 ms).
//
//   reference                                              here
//   fsm::Driver::run  (fsm.rs:51-88)                       BatchedEventLoop::on_instruction
//     Notify -> notifications[block_id] = (addr, req id)     notifications_[{group, block_id}]
//     Apply  -> skip block 0; fsm.transition(data); if a     fsm(group, data); a pending notification
//               notification is pending, ClientResponse        completes the client's request
//               {id, res} to that address via rpc_tx           (the hop rpc_tx -> event_loop ->
//                                                              oneshot of server.rs:144-152 is direct)
//   server::event_loop (server.rs:103-165)                 BatchedEventLoop::run_until
//     step_interval.tick() => apply(Tick)                    one Tick per partition per TICK_MS
//     tcp_rx.recv()        => apply(msg.command)             tcp_rx(msg): queued, applied at the next step
//     rpc_rx.recv(): Peer / Peers => tcp_tx.send(msg)        tcp_tx sink
//                    Local        => apply(msg.command)      re-submitted in the same step
//                    Client       => requests.remove(id)     completes the client's request
//     client_rx.recv()     => apply(ClientRequest{new id})   propose(group, proposal, on_response)
class BatchedEventLoop {
 public:
  static constexpr uint64_t TICK_MS = 100;  // server.rs:25
  using Response = std::function<void(bool ok, const std::vector<uint8_t>& res)>;
  // Fsm::transition (fsm.rs:16): state machine of one partition; an exception is a ResponseError
  std::function<std::vector<uint8_t>(uint32_t group, const std::vector<uint8_t>& data)> fsm;
  std::function<void(const Message&)> tcp_tx;  // to the peer transport (tcp.rs), by partition
  // What the interval's Tick is (server.rs:125): JG_NODE_TICK through jg_step_node - ONE flag for all
  // partitions, the inbound rows classified and served by the dense kernels on the device - or, with
  // dense = false, one Tick row per partition through jg_submit + jg_step (the general state machine only:
  // round 2's loop, kept for the A/B in tests/cpp/bench_event_loop.cpp).
  bool dense = true;
  uint32_t halves = JG_NODE_LEADER_HALF | JG_NODE_FOLLOWER_HALF;
  // ONE loop that overlaps with itself: a step returns as soon as its rows are on the device and classified; what it
  // pushed on fsm_tx / rpc_tx is delivered at the start of the NEXT step (or by flush()) - the channels of the
  // reference are asynchronous too (mod.rs:337-340) -, so that the transport decodes tick t + 1 into the engine's
  // pinned columns while the device runs tick t's kernels and sends its outputs home.
  bool pipelined = false;
  // ... with TWO ticks in flight (2; needs pipelined): what step t pushed on fsm_tx / rpc_tx is delivered at the start of
  // step t + 2 - step t + 1, begun a tick ago, keeps the device busy meanwhile (JG_NODE_KEEP: the engine keeps a step's
  // outbox and rows in a set of its own until they have been viewed, and a view waits for ITS step only) - so that a tick's
  // whole chain (rows up, kernels, columns and fsm rows down: ~3 ms at 1 M x 5) has two periods to complete and the loop's
  // period is its slowest stage (the transport's decoding + the sinks, the bus one way, the bus the other way), not their
  // sum.  The channels of the reference promise an order, not a latency (mod.rs:337-340): every channel carries the same
  // rows in the same order per step, one step later than with 1.
  uint32_t in_flight = 1;
  // the node step's compact bus formats (ABI v7): JG_NODE_COMMON_AE - the Tick's AppendEntries words come home as one
  // word per partition where the followers' agree - and / or JG_NODE_FSM_FUSED - a leader's fsm_tx rows of a step as one
  // row; both are expanded again by BatchedRaft before rpc_tx / fsm_tx see them (a column / row sink sees the compact form)
  uint32_t bus = 0;
  // The feeds of a loop with two ticks in flight (ABI v21; only a caller of set_poll needs a library that has
  // jg_step_node_polled / jg_node_poll_view): with in_flight >= 2 every tick's step carries `q` (under the time rule with the
  // step's own time as clock.now_ms), and `sink` receives the PollResult when that tick's outputs are consumed - after its
  // fsm_tx / rpc_tx rows and columns.  A template, so that a program that never polls does not name the entry points.
  using PollSink = std::function<void(const BatchedRaft::PollResult&, bool redone)>;
  template <class Raft = BatchedRaft>
  void set_poll(const typename Raft::PollRequest& q, PollSink sink) {
    Raft* const r = &raft_;
    poll_q_ = std::make_shared<BatchedRaft::PollRequest>(q);
    begin_polled_ = [r, q](uint64_t at, uint32_t flags) {
      typename Raft::PollRequest qq = q;
      if (qq.timed) qq.clock.now_ms = at;
      r->step_node_polled(at, flags, qq);
    };
    view_polled_ = [r, sink]() {
      bool polled = false, redone = false;
      const typename Raft::PollResult res = r->node_poll(&polled, &redone);
      if (polled && sink) sink(res, redone);
    };
  }

  // The completion feed of a loop with two ticks in flight (ABI v23; only a caller of set_completions needs a library that
  // has jg_step_node_awaited / jg_node_await_view): with in_flight >= 2 every tick's step registers the waiters `source`
  // hands over for it - called when the step begins, with the step's time - and watches at that time; `sink` receives the
  // done rows when that tick's outputs are consumed, after the poll's sink.  The poll of set_poll, if any, travels with the
  // same step.  `limit`: the rows a tick takes (what is left is pending at the next).
  using CompletionSource = std::function<std::vector<jg_await_row>(uint64_t now_ms)>;
  using CompletionSink = std::function<void(const std::vector<jg_done_row>&, bool redone)>;
  template <class Raft = BatchedRaft>
  void set_completions(CompletionSource source, CompletionSink sink, size_t limit = SIZE_MAX) {
    Raft* const r = &raft_;
    fill_awaited_ = [this, source, limit](uint64_t at, BatchedRaft::AwaitRequest& a) {
      if (source) a.rows = source(at);
      a.now_ms = at, a.limit = limit;
      if (!cancels_.empty()) {  // cancel_tokens: the oldest key set travels with this step
        a.cancel_keys.swap(cancels_.front().first), a.cancel_mask = cancels_.front().second;
        cancels_.pop_front();
      }
    };
    begin_awaited_ = [this, r](uint64_t at, uint32_t flags) {
      typename Raft::AwaitRequest a;
      fill_awaited_(at, a);
      BatchedRaft::PollRequest qq;
      if (poll_q_) {
        qq = *poll_q_;
        if (qq.timed) qq.clock.now_ms = at;
      }
      r->step_node_awaited(at, flags, poll_q_ ? &qq : nullptr, a);
    };
    view_awaited_ = [r, sink]() {
      bool attached = false, redone = false;
      const typename Raft::Completions c = r->node_completions(&attached, &redone);
      if (attached && sink) sink(c.rows, redone);
    };
  }

  // Point queries from inside the loop (ABI v25; only a caller of lookup_async needs a library that has jg_step_node_looked /
  // jg_node_lookup_view): the state of `groups` (any order, repeats allowed, at most JG_NODE_LOOKUP_MAX; with `progress` the
  // progress heads too) - what Metadata, ListOffsets and a produce pre-check ask on a client connection.  Requests queue up.
  // With in_flight >= 2 every tick's step carries the oldest one - and the ones behind it while their `progress` agrees and
  // they fit JG_NODE_LOOKUP_MAX together, each sink getting its own slice - beside the poll of set_poll and the completion
  // request of set_completions; the sink is called when that tick's outputs are consumed, after the poll's and the
  // completions' sinks, with the partitions as that tick's step left them.  On a loop below two in flight no step is kept:
  // the request is answered by the synchronous BatchedRaft::lookup at the next step boundary.
  using LookupSink = std::function<void(const BatchedRaft::GroupStates&, bool redone)>;
  template <class Raft = BatchedRaft>
  void lookup_async(std::vector<uint32_t> groups, bool progress, LookupSink sink) {
    if (groups.size() > JG_NODE_LOOKUP_MAX) throw EngineError(JG_EINVAL, "lookup_async: more than JG_NODE_LOOKUP_MAX entries");
    lookups_.push_back(LookupAsk{std::move(groups), progress, std::move(sink)});
    if (begin_looked_) return;
    Raft* const r = &raft_;
    begin_looked_ = [this, r](uint64_t at, uint32_t flags, bool awaited) {
      std::vector<uint32_t> list;
      std::vector<LookupSlice> slices;
      bool progress = false;
      const size_t take = gather_lookups(list, slices, progress);
      typename Raft::AwaitRequest a;
      if (awaited) fill_awaited_(at, a);
      BatchedRaft::PollRequest qq;
      if (poll_q_) {
        qq = *poll_q_;
        if (qq.timed) qq.clock.now_ms = at;
      }
      r->step_node_looked(at, flags, poll_q_ ? &qq : nullptr, awaited ? &a : nullptr, list.data(), list.size(), progress);
      lookups_.erase(lookups_.begin(), lookups_.begin() + (std::ptrdiff_t)take);  // (a refused step keeps its requests queued)
      looked_slices_.push_back(std::move(slices));
    };
    view_looked_ = [this, r]() {
      bool attached = false, redone = false;
      const typename Raft::GroupStates all = r->node_lookup(&attached, &redone);
      std::vector<LookupSlice> slices;
      slices.swap(looked_slices_.front());
      looked_slices_.pop_front();
      if (!attached) return;
      const size_t R = all.rows.empty() ? 0 : all.match.size() / all.rows.size();
      for (const LookupSlice& s : slices) {
        if (!s.sink) continue;
        if (slices.size() == 1) {
          s.sink(all, redone);
          continue;
        }
        typename Raft::GroupStates part;
        part.rows.assign(all.rows.begin() + (std::ptrdiff_t)s.at, all.rows.begin() + (std::ptrdiff_t)(s.at + s.n));
        if (R) part.match.assign(all.match.begin() + (std::ptrdiff_t)(s.at * R), all.match.begin() + (std::ptrdiff_t)((s.at + s.n) * R));
        s.sink(part, redone);
      }
    };
    sync_looked_ = [this, r]() {  // (nothing is outstanding: the synchronous call, request by request)
      while (!lookups_.empty()) {
        const LookupAsk q = std::move(lookups_.front());
        lookups_.pop_front();
        const typename Raft::GroupStates res = r->lookup(q.groups.data(), q.groups.size(), q.progress);
        if (q.sink) q.sink(res, false);
      }
    };
  }

  // Partitions opened and closed from inside the loop (ABI v26; only a caller of open_async / close_async needs a library that
  // has jg_step_node_hosted / jg_node_hosting_view): what LeaderAndIsr, CreateTopics, DeleteTopics and the last step of a
  // partition move do in a running broker.  `groups` strictly ascending, at most JG_NODE_HOSTING_MAX; `self_slots` empty (every
  // slot keeps its own) or one own slot per group.  Requests queue up.  With in_flight >= 2 every tick's step carries the
  // oldest close and the oldest open - the close is made first, so a step may close and reopen a slot - beside the poll, the
  // completion request and the point queries; a sink is called when that tick's outputs are consumed, after the lookups'
  // sinks, the two of one step in the order they were asked: applied == false - a listed slot was in the wrong state, the
  // set wrote nothing.  Rows for a slot that a tick opens may be handed to the loop from the next tick on.  On a loop below
  // two in flight no step is kept: the requests are made by the synchronous BatchedRaft::close_groups / open_groups at the
  // next step boundary, in the order they were asked - applied == false, as from a step, where a listed slot is in the wrong
  // state (the loop asks first); anything else that refuses the synchronous call throws out of run_until.  A request the
  // step could not carry is refused by open_async / close_async themselves: a list too long, not ascending or out of range,
  // an own slot >= the number of replicas.
  using HostingSink = std::function<void(bool applied, bool redone)>;
  template <class Raft = BatchedRaft>
  void open_async(std::vector<uint32_t> groups, std::vector<uint8_t> self_slots, HostingSink sink) {
    if (!self_slots.empty() && self_slots.size() != groups.size()) throw EngineError(JG_EINVAL, "open_async: one own slot per group, or none");
    hosting_ask<Raft>(opens_, "open_async", std::move(groups), std::move(self_slots), std::move(sink));
  }
  template <class Raft = BatchedRaft>
  void close_async(std::vector<uint32_t> groups, HostingSink sink) {
    hosting_ask<Raft>(closes_, "close_async", std::move(groups), {}, std::move(sink));
  }

  // Withdraw waiters from inside the loop (ABI v24; with set_completions): the keys are attached to the next awaited tick's
  // step - registered, cancelled, watched, in that order - and the withdrawn waiters reach the sink as JG_DONE_CANCELLED rows.
  // Calls with the same mask before that tick are merged into one key set (while it stays within JG_AWAIT_CANCEL_MAX); a
  // different mask starts a key set of its own, for the tick after.  Only awaited ticks carry a cancel: without
  // set_completions the call throws, and on a loop whose in_flight is below 2 - no tick is awaited there - the keys wait
  // until it is raised; such a loop cancels with BatchedRaft::cancel_waiters between its ticks.
  void cancel_tokens(const std::vector<uint64_t>& keys, uint64_t mask = UINT64_MAX) {
    if (!begin_awaited_) throw EngineError(JG_EINVAL, "cancel_tokens: no awaited ticks (set_completions first)");
    if (keys.empty()) return;
    if (!cancels_.empty() && cancels_.back().second == mask && cancels_.back().first.size() + keys.size() <= JG_AWAIT_CANCEL_MAX)
      cancels_.back().first.insert(cancels_.back().first.end(), keys.begin(), keys.end());
    else
      cancels_.emplace_back(keys, mask);
  }

  explicit BatchedEventLoop(BatchedRaft& raft, uint32_t n_groups) : raft_(raft), G_(n_groups), answers_to_(n_groups, 0) {
    raft_.rpc_tx = [this](const Message& m) { on_message(m); };
    raft_.fsm_tx = [this](const Instruction& i) { on_instruction(i); };
  }
  // a message from a peer's event loop (tcp_rx, server.rs:126-137): queued as a ROW (structure of arrays),
  // applied at the next step; block payloads go to the partition's store when the step has extended the chain
  void tcp_rx(const Message& m) {
    const Command& c = m.command;
    if (c.kind == JG_CMD_APPEND_ENTRIES) {
      in_.push_append_entries(m.group, c.from, c.term, c.blocks.data(), c.blocks.size());
      for (const Block& b : c.blocks) in_blocks_.push_back({m.group, b});
    } else {
      // (a HeartbeatResponse does not name its sender in the Command; the Message does: rpc.rs:17-27)
      const NodeId from = c.kind == JG_CMD_HEARTBEAT_RESPONSE ? m.from.peer : c.from;
      in_.push(m.group, c.kind, from, c.term, c.id, c.aux, c.flag ? 1 : 0);
      if (c.kind == JG_CMD_CLIENT_REQUEST) proxied_[{m.group, c.id}] = c.proposal;
    }
    // (who a partition's answers go to - the sender of the Heartbeat / AppendEntries being answered - is read off the
    // row queue when the step that applies it begins: step(); a pipelined loop decodes tick t + 1 while tick t's
    // answers are still to be addressed)
  }
  // a peer's whole frame of rows at once (payload-free: a columnar transport ships block data separately)
  void tcp_rx_rows(const jg_cmd_batch& b) { in_.append(b); }
  // ... or decoded straight into the engine's pinned columns: no copy on the host at all (rows committed this
  // way are applied before the rows queued through tcp_rx / tcp_rx_rows of the same step)
  jg_cmd_cols tcp_rx_reserve(size_t n, size_t n_blocks = 0) { return raft_.reserve_rows(n, n_blocks); }
  void tcp_rx_commit(size_t n, size_t n_blocks, uint32_t optional_columns) {
    raft_.commit_rows(n, n_blocks, optional_columns);
    direct_rows_ += n;
  }
  // ... and a batched peer ships its answers as the COLUMN it produced (jg_node_outbox.answer): 8 bytes per partition
  // instead of two rows; filled in place, applied by the next step's leader half (hb_commit == nullptr: not needed)
  void tcp_rx_answer_column(uint32_t peer_slot, uint64_t** answer, uint64_t** hb_commit) {
    raft_.inbox_columns(peer_slot, answer, hb_commit);
    direct_rows_ += 1;  // (something to apply even without a Tick)
  }
  // RaftClient::propose (client.rs:35): returns the request id (Uuid::new_v4 -> a counter)
  uint64_t propose(uint32_t group, std::vector<uint8_t> proposal, Response on_response) {
    const uint64_t id = ++next_request_;
    requests_[id] = std::move(on_response);
    in_.push(group, JG_CMD_CLIENT_REQUEST, 0, 0, id, 0, 0);
    proposals_.push_back({group, id, std::move(proposal)});
    return id;
  }
  // Advance logical time to now_ms: everything that arrived is applied, a Tick per partition
  // whenever the interval fires (the first one immediately, like tokio::time::interval).
  void run_until(uint64_t now_ms) {
    for (;;) {
      const bool tick = next_tick_ <= now_ms;
      const uint64_t at = tick ? next_tick_ : now_ms;
      if (!tick && in_.empty() && !direct_rows_) break;
      step(at, tick);
      if (tick) next_tick_ += TICK_MS;
    }
  }
  // pipelined: deliver what the last step pushed on fsm_tx / rpc_tx (run_until does it at the start of the next step)
  void flush() {
    while (raft_.node_step_open()) finish_oldest();
    drain_local(last_at_);
  }
  size_t pending_requests() const { return requests_.size(); }
  size_t queued_rows() const { return in_.size(); }

 private:
  void step(uint64_t at, bool tick) {
    // (pipelined: the previous step's outputs first - its pinned queues and outbox are about to be reused, the blocks
    // noted below belong to THIS step (BatchedRaft::after_step stores a step's blocks where its extend succeeded), and
    // its answers go to the senders of ITS Heartbeat / AppendEntries rows, not to this step's)
    const bool two = dense && pipelined && in_flight >= 2;
    if (two) {
      // two ticks in flight: what the step BEFORE LAST pushed on the channels is delivered now - its outputs have had this
      // long to travel home - while the last step, begun a tick ago, keeps the device busy
      while (raft_.node_steps_open() >= 2) finish_oldest();
      if (!local_.empty()) flush();  // (Address::Local messages are applied by a step of their own: nothing may be in flight)
    } else if (dense) {
      flush();
    }
    if (!two && sync_looked_ && !lookups_.empty()) sync_looked_();  // (a step boundary of a loop that keeps no step)
    if (!two && sync_hosted_ && (!closes_.empty() || !opens_.empty())) sync_hosted_(at);
    // (who THIS step's answers go to: noted per step, applied when the step is finished - with two ticks in flight the
    // step before is finished after this one has begun, and its answers go to the senders of ITS rows)
    std::vector<std::pair<uint32_t, NodeId>> answers;
    for (size_t i = 0; dense && i < in_.size(); i++)
      if (in_.kind[i] == JG_CMD_HEARTBEAT || in_.kind[i] == JG_CMD_APPEND_ENTRIES) answers.push_back({in_.group[i], in_.from[i]});
    // payload-carrying rows (client proposals, blocks) go through submit() so that BatchedRaft's request /
    // block mirrors see them; everything else is one bulk jg_submit of the row queue
    for (auto& p : proposals_) raft_.note_proposal(p.group, p.id, std::move(p.data));
    proposals_.clear();
    for (auto& kv : proxied_) raft_.note_proposal(kv.first.first, kv.first.second, kv.second);
    proxied_.clear();
    for (auto& pb : in_blocks_) raft_.note_block(pb.first, pb.second);
    in_blocks_.clear();
    direct_rows_ = 0;
    if (dense) {
      if (!in_.empty()) raft_.submit_rows(in_.view());
      in_.clear();
      const bool awaited = two && begin_awaited_;  // (the step with both attachments, if there is a poll)
      const bool polled = two && (begin_polled_ || (awaited && poll_q_));
      const bool looked = two && begin_looked_ && !lookups_.empty();  // (... and the point queries that are waiting)
      const bool hosted = two && begin_hosted_ && (!closes_.empty() || !opens_.empty());  // (... and the oldest close and open)
      if (hosted) begin_hosted_(at, halves | bus | (tick ? (uint32_t)JG_NODE_TICK : 0u), awaited, looked);
      else if (looked) begin_looked_(at, halves | bus | (tick ? (uint32_t)JG_NODE_TICK : 0u), awaited);
      else if (awaited) begin_awaited_(at, halves | bus | (tick ? (uint32_t)JG_NODE_TICK : 0u));
      else if (polled) begin_polled_(at, halves | bus | (tick ? (uint32_t)JG_NODE_TICK : 0u));
      else raft_.step_node_begin(at, halves | bus | (tick ? (uint32_t)JG_NODE_TICK : 0u), pipelined, two);
      polled_steps_.push_back(polled);
      awaited_steps_.push_back(awaited);
      looked_steps_.push_back(looked);
      hosted_steps_.push_back(hosted);
      answers_of_step_.push_back(std::move(answers));  // (once the step has begun: one entry per open step, whatever begin() throws)
      last_at_ = at;
      if (pipelined) return;
      finish_oldest();
    } else {
      if (tick)
        for (uint32_t g = 0; g < G_; g++) in_.push(g, JG_CMD_TICK);
      if (!in_.empty()) raft_.submit_rows(in_.view());
      in_.clear();
      raft_.step(at);
    }
    drain_local(at);
  }
  void finish_oldest() {
    if (!answers_of_step_.empty()) {
      for (const auto& u : answers_of_step_.front()) answers_to_[u.first] = u.second;
      answers_of_step_.pop_front();
    }
    raft_.step_node_finish(&answers_to_);
    if (!polled_steps_.empty()) {
      const bool polled = polled_steps_.front();
      polled_steps_.pop_front();
      if (polled) view_polled_();
    }
    if (!awaited_steps_.empty()) {
      const bool awaited = awaited_steps_.front();
      awaited_steps_.pop_front();
      if (awaited) view_awaited_();
    }
    if (!looked_steps_.empty()) {
      const bool looked = looked_steps_.front();
      looked_steps_.pop_front();
      if (looked) view_looked_();
    }
    if (!hosted_steps_.empty()) {
      const bool hosted = hosted_steps_.front();
      hosted_steps_.pop_front();
      if (hosted) view_hosted_();
    }
  }
  // Address::Local messages (server.rs:143) are applied before anything new is accepted
  void drain_local(uint64_t at) {
    int guard = 0;
    while (!local_.empty() && guard++ < 64) {
      std::deque<Message> lo;
      lo.swap(local_);
      for (const Message& m : lo) raft_.submit(m.group, m.command);
      raft_.step(at);
    }
  }
  void on_message(const Message& m) {  // rpc_rx (server.rs:139-155)
    switch (m.to.kind) {
      case JG_TO_PEER:
      case JG_TO_PEERS:
        if (tcp_tx) tcp_tx(m);
        break;
      case JG_TO_LOCAL: local_.push_back(m); break;
      case JG_TO_CLIENT: complete(m.command.id, true, {}); break;
      default: throw EngineError(JG_EINVAL, "unexpected message");  // server.rs:154
    }
  }
  void on_instruction(const Instruction& i) {  // fsm.rs:56-84
    const std::pair<uint32_t, BlockId> key{i.group, i.kind == Instruction::Notify ? i.block_id : i.block.id};
    if (i.kind == Instruction::Notify) {
      notifications_[key] = i.request_id;
      return;
    }
    if (i.block.id == 0) return;  // fsm.rs:59-61
    bool ok = true;
    std::vector<uint8_t> res;
    try {
      if (fsm) res = fsm(i.group, i.block.data);
    } catch (...) {
      ok = false;
    }
    auto it = notifications_.find(key);
    if (it != notifications_.end()) {
      complete(it->second, ok, res);
      notifications_.erase(it);
    }
  }
  void complete(uint64_t id, bool ok, const std::vector<uint8_t>& res) {
    auto it = requests_.find(id);
    if (it == requests_.end()) return;  // a proxied request: its oneshot lives on another node (server.rs:129-133)
    Response cb = std::move(it->second);
    requests_.erase(it);
    if (cb) cb(ok, res);
  }

  struct Proposal {
    uint32_t group;
    uint64_t id;
    std::vector<uint8_t> data;
  };
  BatchedRaft& raft_;
  uint32_t G_;
  uint64_t next_tick_ = 0, next_request_ = 0, last_at_ = 0;
  size_t direct_rows_ = 0;                                // rows committed in place since the last step
  RowQueue in_;                                           // tcp_rx + client_rx since the last step, stream order
  std::vector<std::pair<uint32_t, Block>> in_blocks_;     // payloads of the AppendEntries rows in in_
  std::vector<Proposal> proposals_;                       // payloads of the ClientRequest rows in in_
  std::map<std::pair<uint32_t, uint64_t>, std::vector<uint8_t>> proxied_;
  std::vector<NodeId> answers_to_;                        // per partition: who its Heartbeat / AppendEntries came from
  std::deque<std::vector<std::pair<uint32_t, NodeId>>> answers_of_step_;  // ... as noted by the steps begun and not finished
  std::function<void(uint64_t, uint32_t)> begin_polled_;  // set_poll: the step with the request attached ...
  std::function<void()> view_polled_;                      // ... and its answer to the sink
  std::deque<bool> polled_steps_;                          // per open step: was it begun with the poll
  std::shared_ptr<BatchedRaft::PollRequest> poll_q_;       // set_poll's request: an awaited step carries it along
  std::function<void(uint64_t, uint32_t)> begin_awaited_;  // set_completions: the step with the request(s) attached ...
  std::function<void()> view_awaited_;                     // ... and its done rows to the sink
  std::deque<std::pair<std::vector<uint64_t>, uint64_t>> cancels_;  // cancel_tokens: (keys, mask) per awaited tick to come
  std::deque<bool> awaited_steps_;                         // per open step: was it begun with the completion request
  std::function<void(uint64_t, BatchedRaft::AwaitRequest&)> fill_awaited_;  // set_completions: the request of the step beginning at a time
  struct LookupAsk {
    std::vector<uint32_t> groups;
    bool progress;
    LookupSink sink;
  };
  struct LookupSlice {
    size_t at, n;  // the request's entries among the step's
    LookupSink sink;
  };
  std::deque<LookupAsk> lookups_;                          // lookup_async: the requests no step carries yet, oldest first
  std::function<void(uint64_t, uint32_t, bool)> begin_looked_;  // lookup_async: the step with the lookup (and the other requests) attached ...
  std::function<void()> view_looked_;                      // ... its rows to the sinks ...
  std::function<void()> sync_looked_;                      // ... and the requests of a loop that keeps no step, answered synchronously
  std::deque<bool> looked_steps_;                          // per open step: was it begun with a lookup
  std::deque<std::vector<LookupSlice>> looked_slices_;     // per looked step: whose entries are where
  struct HostingAsk {
    uint64_t asked;  // the request's number among the loop's hosting requests
    std::vector<uint32_t> groups;
    std::vector<uint8_t> self_slots;
    HostingSink sink;
  };
  struct HostedStep {
    bool has_close = false, has_open = false;
    uint64_t close_asked = 0, open_asked = 0;
    HostingSink close, open;
  };
  std::deque<HostingAsk> closes_, opens_;                  // close_async / open_async: the requests no step carries yet, oldest first
  uint64_t hosting_asked_ = 0;
  std::function<void(uint64_t, uint32_t, bool, bool)> begin_hosted_;  // open_async / close_async: the step with the hosting request (and the other requests) attached ...
  std::function<void()> view_hosted_;                      // ... its verdict to the sinks ...
  std::function<void(uint64_t)> sync_hosted_;              // ... and the requests of a loop that keeps no step, made synchronously
  std::deque<bool> hosted_steps_;                          // per open step: was it begun with a hosting request
  std::deque<HostedStep> hosted_sinks_;                    // per hosted step: who hears of which set
  // lookup_async: the oldest request and whoever behind it travels along - their entries into `list`, who gets which into
  // `slices`; returns how many requests these are (they stay queued: a refused step keeps them)
  size_t gather_lookups(std::vector<uint32_t>& list, std::vector<LookupSlice>& slices, bool& progress) const {
    progress = lookups_.front().progress;
    size_t take = 0;
    for (const LookupAsk& q : lookups_) {
      if (take && (q.progress != progress || list.size() + q.groups.size() > JG_NODE_LOOKUP_MAX)) break;
      slices.push_back(LookupSlice{list.size(), q.groups.size(), q.sink});
      list.insert(list.end(), q.groups.begin(), q.groups.end());
      take++;
    }
    return take;
  }
  // open_async / close_async: the request checked (what would refuse the step that carries it refuses the call) and queued
  template <class Raft>
  void hosting_ask(std::deque<HostingAsk>& queue, const char* who, std::vector<uint32_t> groups, std::vector<uint8_t> self_slots, HostingSink sink) {
    if (groups.size() > JG_NODE_HOSTING_MAX) throw EngineError(JG_EINVAL, (std::string(who) + ": more than JG_NODE_HOSTING_MAX entries").c_str());
    for (size_t i = 0; i < groups.size(); i++)
      if (groups[i] >= G_ || (i && groups[i - 1] >= groups[i])) throw EngineError(JG_EINVAL, (std::string(who) + ": slot indices strictly ascending and within the engine").c_str());
    for (uint8_t s : self_slots)
      if (s >= raft_.replicas()) throw EngineError(JG_EINVAL, (std::string(who) + ": an own slot >= the number of replicas").c_str());
    queue.push_back(HostingAsk{hosting_asked_++, std::move(groups), std::move(self_slots), std::move(sink)});
    if (begin_hosted_) return;
    Raft* const r = &raft_;
    begin_hosted_ = [this, r](uint64_t at, uint32_t flags, bool awaited, bool looked) {
      std::vector<uint32_t> list;
      std::vector<LookupSlice> slices;
      bool progress = false;
      const size_t take = looked ? gather_lookups(list, slices, progress) : 0;
      typename Raft::AwaitRequest a;
      if (awaited) fill_awaited_(at, a);
      BatchedRaft::PollRequest qq;
      if (poll_q_) {
        qq = *poll_q_;
        if (qq.timed) qq.clock.now_ms = at;
      }
      typename Raft::Hosting h;
      HostedStep sinks;
      if (!closes_.empty()) h.has_close = true, h.close = closes_.front().groups, sinks.close = closes_.front().sink, sinks.close_asked = closes_.front().asked;
      if (!opens_.empty()) {
        const HostingAsk& o = opens_.front();
        h.has_open = true, h.open = o.groups, h.has_self = !o.self_slots.empty(), h.self_slots = o.self_slots;
        sinks.open = o.sink, sinks.open_asked = o.asked;
      }
      sinks.has_close = h.has_close, sinks.has_open = h.has_open;
      r->step_node_hosted(at, flags, poll_q_ ? &qq : nullptr, awaited ? &a : nullptr, looked, list.data(), list.size(), progress, h);
      // (a refused step keeps its requests queued)
      if (looked) lookups_.erase(lookups_.begin(), lookups_.begin() + (std::ptrdiff_t)take), looked_slices_.push_back(std::move(slices));
      if (h.has_close) closes_.pop_front();
      if (h.has_open) opens_.pop_front();
      hosted_sinks_.push_back(std::move(sinks));
    };
    view_hosted_ = [this, r]() {
      const typename Raft::HostingVerdict v = r->node_hosting();
      const HostedStep s = std::move(hosted_sinks_.front());
      hosted_sinks_.pop_front();
      if (!v.attached) return;
      const bool close_first = !s.has_open || (s.has_close && s.close_asked < s.open_asked);
      for (int k = 0; k < 2; k++) {
        const bool close = (k == 0) == close_first;
        if (close && s.has_close && s.close) s.close(!v.close_refused, v.redone);
        if (!close && s.has_open && s.open) s.open(!v.open_refused, v.redone);
      }
    };
    sync_hosted_ = [this, r](uint64_t at) {  // (nothing is outstanding: the synchronous calls, in the order they were asked)
      while (!closes_.empty() || !opens_.empty()) {
        const bool close = opens_.empty() || (!closes_.empty() && closes_.front().asked < opens_.front().asked);
        std::deque<HostingAsk>& queue = close ? closes_ : opens_;
        const HostingAsk q = std::move(queue.front());
        queue.pop_front();
        // (a listed slot in the wrong state - what a step reports as refused - is found by asking; whatever else refuses the
        // call, commands that are still queued for instance, is the caller's to hear of: it throws)
        bool applied = true;
        if (!q.groups.empty()) {
          const typename Raft::GroupStates now = r->lookup(q.groups.data(), q.groups.size(), false);
          for (const jg_group_state& s : now.rows) applied = applied && (s.fault == JG_FAULT_VACANT) == !close;
        }
        if (applied) {
          if (close) r->close_groups(q.groups);
          else r->open_groups(q.groups, at, q.self_slots.empty() ? nullptr : &q.self_slots);
        }
        if (q.sink) q.sink(applied, false);
      }
    };
  }
  std::deque<Message> local_;
  std::map<uint64_t, Response> requests_;
  std::map<std::pair<uint32_t, BlockId>, uint64_t> notifications_;
};

inline RaftHandle RaftHandle::apply(const Command& cmd, uint64_t now_ms) { return e_->apply(g_, cmd, now_ms); }
inline uint64_t RaftHandle::read64(int f) const {
  uint64_t v = 0;
  e_->check(jg_read_state(e_->e_, f, 0, &v, g_, 1));
  return v;
}
inline uint32_t RaftHandle::read32(int f) const {
  uint32_t v = 0;
  e_->check(jg_read_state(e_->e_, f, 0, &v, g_, 1));
  return v;
}
inline uint8_t RaftHandle::read8(int f) const {
  uint8_t v = 0;
  e_->check(jg_read_state(e_->e_, f, 0, &v, g_, 1));
  return v;
}

}  // namespace josefine
