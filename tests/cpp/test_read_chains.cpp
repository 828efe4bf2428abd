// The engine's chain trees against the C++ host mirror's stores: an in-process 3-node cluster (three instances of one
// partition in one BatchedRaft, the examples/multi-node ids 1, 2, 3) elects and commits; each node's read_chains
// (jg_engine_read_chains) must be its BlockStore - the same block keys, the same parents, the same "commit" key.  Then
// the process dies, BatchedRaft::open brings it back on the stores' raw bytes, and the read must be the stores again.
// Built and run by tests/test_cpp_read_chains.py (-m gpu).
#include <cstdio>
#include <deque>
#include <memory>

#include "../../josefine_amd/host/formats.hpp"  // (includes raft_handle.hpp)

using namespace josefine;

static int g_failed = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                                    \
    }                                                                                \
  } while (0)

static const uint8_t kSlots[3] = {0, 1, 2};

static void deliver_all(BatchedRaft& raft, std::deque<Message>& wire, uint64_t now) {
  int guard = 0;
  while (!wire.empty() && guard++ < 1000) {
    const Message m = wire.front();
    wire.pop_front();
    for (uint32_t dst = 0; dst < 3; dst++) {
      const NodeId id = dst + 1;
      if ((m.to.kind == JG_TO_PEERS && id != m.from.peer) || (m.to.kind == JG_TO_PEER && m.to.peer == id)) raft.apply(dst, m.command, now);
    }
  }
}

// node g's read == a scan of its store: keys (8-byte block ids) in order with each Block.next, and the commit key
static void check_read_is_store(BatchedRaft& raft, const char* what) {
  const BatchedRaft::ChainRows c = raft.read_chains();
  CHECK(c.off.size() == 4);
  for (uint32_t g = 0; g < 3; g++) {
    std::vector<uint64_t> ids, nexts;
    bool has = false;
    uint64_t commit = 0;
    for (const auto& kv : raft.store(g).raw()) {
      if (kv.first == formats::ChainStore::commit_key()) {
        has = true;
        commit = formats::key_block_id(kv.second);
      } else if (kv.first.size() == 8) {
        ids.push_back(formats::key_block_id(kv.first));
        nexts.push_back(formats::decode_block(kv.second).next);
      }
    }
    const std::vector<uint64_t> got_ids(c.id.begin() + c.off[g], c.id.begin() + c.off[g + 1]);
    const std::vector<uint64_t> got_next(c.next.begin() + c.off[g], c.next.begin() + c.off[g + 1]);
    const bool same = got_ids == ids && got_next == nexts && (c.has_commit[g] != 0) == has && c.commit[g] == commit && c.fault[g] == 0;
    if (!same) {
      std::fprintf(stderr, "%s: node %u: engine %zu blocks (commit key %d: %llu), store %zu blocks (commit key %d: %llu)\n", what, g,
                   got_ids.size(), (int)c.has_commit[g], (unsigned long long)c.commit[g], ids.size(), (int)has, (unsigned long long)commit);
      for (size_t k = 0; k < std::max(got_ids.size(), ids.size()); k++)
        std::fprintf(stderr, "   engine %s  store %s\n",
                     k < got_ids.size() ? (std::to_string(got_ids[k]) + "<-" + std::to_string(got_next[k])).c_str() : "-",
                     k < ids.size() ? (std::to_string(ids[k]) + "<-" + std::to_string(nexts[k])).c_str() : "-");
    }
    CHECK(same);
  }
}

int main() {
  try {
    std::deque<Message> wire;
    std::vector<std::map<formats::Bytes, formats::Bytes>> disk(3);
    {
      BatchedRaft raft(3, {1, 2, 3}, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY);
      raft.rpc_tx = [&](const Message& m) { wire.push_back(m); };
      if (jg_set_self_slots(raft.raw(), kSlots) != JG_OK) throw std::runtime_error("jg_set_self_slots");
      check_read_is_store(raft, "fresh");
      raft.apply(0, Command::Timeout());  // node 1 campaigns and wins
      deliver_all(raft, wire, 0);
      CHECK(raft.handle(0).is_leader());
      uint64_t now = 0;
      for (uint8_t k = 1; k <= 3; k++) {  // three proposals, replicated and committed everywhere
        raft.apply(0, Command::ClientRequest(k, {k}), now += 10);
        raft.apply(0, Command::Tick(), now += 10);
        deliver_all(raft, wire, now);
        raft.apply(0, Command::Tick(), now += 150);  // heartbeat: carries the commit
        deliver_all(raft, wire, now);
      }
      for (uint32_t g = 0; g < 3; g++) CHECK(raft.handle(g).commit() == 3 && raft.store(g).commit() == 3);
      check_read_is_store(raft, "committed");
      // a block beyond the commit on one follower
      Block b;
      b.id = 4, b.next = 3, b.data = {4};
      raft.apply(1, Command::AppendEntries(1, 1, {b}), now += 10);
      check_read_is_store(raft, "one block ahead");
      for (uint32_t g = 0; g < 3; g++) disk[g] = raft.store(g).raw();
      wire.clear();
    }  // the process is gone
    std::vector<BlockStore> stores;
    for (uint32_t g = 0; g < 3; g++) stores.push_back(formats::ChainStore::from_raw(disk[g]));
    std::unique_ptr<BatchedRaft> raft = BatchedRaft::open({1, 2, 3}, std::move(stores), 5000, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY, {}, kSlots);
    check_read_is_store(*raft, "reopened");
    const BatchedRaft::ChainRows one = raft->read_chains(1, 1);
    CHECK(one.off.size() == 2 && one.id.size() == 5 && one.id.back() == 4 && one.next.back() == 3 && one.commit[0] == 3);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("read chains ok");
  return 0;
}
