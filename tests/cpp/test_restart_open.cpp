// A broker restart through the C++ host mirror: an in-process 3-node cluster (three instances of one partition in one
// BatchedRaft, the examples/multi-node ids 1, 2, 3) elects and commits; then the process dies - the engine is destroyed
// - and a new one is opened on the stores' raw bytes (ChainStore::from_raw = sled re-opened; BatchedRaft::open =
// Raft::<Follower>::new + Chain::new on each tree, jg_engine_load_chains).  Built and run by
// tests/test_cpp_restart_open.py (-m gpu).
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

// everything on the wire delivered to its addressees (instance g is node g + 1)
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

int main() {
  try {
    std::deque<Message> wire;
    std::vector<std::map<formats::Bytes, formats::Bytes>> disk(3);
    uint64_t commit_before[3];
    {
      BatchedRaft raft(3, {1, 2, 3}, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY);
      raft.rpc_tx = [&](const Message& m) { wire.push_back(m); };
      if (jg_set_self_slots(raft.raw(), kSlots) != JG_OK) throw std::runtime_error("jg_set_self_slots");
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
      for (uint32_t g = 0; g < 3; g++) {
        commit_before[g] = raft.handle(g).commit();
        CHECK(commit_before[g] == 3 && raft.store(g).commit() == 3 && raft.handle(g).fault() == 0);
        disk[g] = raft.store(g).raw();  // what sled holds when the process dies
      }
      // (a block beyond the commit on one follower: it stays in the tree across the restart)
      Block b;
      b.id = 4, b.next = 3, b.data = {4};
      raft.apply(1, Command::AppendEntries(1, 1, {b}), now += 10);
      disk[1] = raft.store(1).raw();
      wire.clear();
    }  // the process is gone
    std::vector<BlockStore> stores;
    for (uint32_t g = 0; g < 3; g++) stores.push_back(formats::ChainStore::from_raw(disk[g]));
    std::unique_ptr<BatchedRaft> raft = BatchedRaft::open({1, 2, 3}, std::move(stores), 5000, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY, {}, kSlots);
    raft->rpc_tx = [&](const Message& m) { wire.push_back(m); };
    for (uint32_t g = 0; g < 3; g++) {
      RaftHandle h = raft->handle(g);
      CHECK(h.is_follower() && h.current_term() == 0 && !h.has_voted() && h.fault() == 0);
      CHECK(h.commit() == raft->store(g).commit() && h.commit() >= commit_before[g]);  // no commit goes backwards
      CHECK(h.head() == h.commit());                                                   // Q8: head = id_gen = commit
    }
    CHECK(raft->store(1).has(4) && raft->store(1).at(4).data == std::vector<uint8_t>{4});  // nothing lost on disk
    // the cluster elects again: node 2 times out and campaigns
    raft->apply(1, Command::Timeout(), 6000);
    deliver_all(*raft, wire, 6000);
    CHECK(raft->handle(1).is_leader() && raft->handle(1).current_term() == 1);
    CHECK(raft->handle(0).is_follower() && raft->handle(2).is_follower());
    for (uint32_t g = 0; g < 3; g++) CHECK(raft->handle(g).commit() >= commit_before[g] && raft->handle(g).fault() == 0);
    // ... and its first append meets Q8 exactly as after JG_CMD_RESTART (Chain::new sets id_gen = commit: the
    // reference asserts id > head, chain.rs:161-163) - the restarted leader's process dies, the commits stay
    raft->apply(1, Command::ClientRequest(9, {9}), 6100);
    CHECK(raft->handle(1).fault() == JG_FAULT_APPEND_ID_NOT_ABOVE_HEAD);
    for (uint32_t g = 0; g < 3; g++) CHECK(raft->handle(g).commit() >= commit_before[g]);
    // that replica restarts once more on its own tree (JG_CMD_RESTART on the adopted store): back at the commit, healthy
    const formats::ChainStore::Reopened r = raft->restart(1, 7000);
    CHECK(r.commit == 3 && raft->handle(1).fault() == 0 && raft->handle(1).commit() == 3 && raft->store(1).has(4));
    for (uint32_t g = 0; g < 3; g++) CHECK(raft->store(g).commit() == 3);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("restart open ok");
  return 0;
}
