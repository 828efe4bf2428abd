// A live hand-over through the C++ host mirror: an in-process 3-node cluster (three instances of one partition in one
// BatchedRaft, the examples/multi-node ids 1, 2, 3) elects and commits; then the leader's instance and its store move to
// a fresh BatchedRaft (BatchedRaft::export_groups / import_groups: jg_engine_export_groups / jg_engine_import_groups) and
// the cluster keeps committing with the same leader and term, and no election - where tests/cpp/test_restart_open.cpp's
// restarted leader faults at its first append (Q8).  A follower with a queued client request moves too: its proposal
// travels with it and is what the leader commits.  Built and run by tests/test_cpp_move_groups.py (-m gpu).
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

// everything on the wire delivered to its addressees: node id i + 1 is instance i of `home[i]` at `at[i]`
struct Route {
  BatchedRaft* home[3];
  uint32_t at[3];
};
static void deliver_all(const Route& rt, std::deque<Message>& wire, uint64_t now) {
  int guard = 0;
  while (!wire.empty() && guard++ < 1000) {
    const Message m = wire.front();
    wire.pop_front();
    for (uint32_t dst = 0; dst < 3; dst++) {
      const NodeId id = dst + 1;
      if ((m.to.kind == JG_TO_PEERS && id != m.from.peer) || (m.to.kind == JG_TO_PEER && m.to.peer == id))
        rt.home[dst]->apply(rt.at[dst], m.command, now);
    }
  }
}

// one proposal on the leader, replicated, then a heartbeat that carries the commit
static void propose(const Route& rt, uint32_t leader, std::deque<Message>& wire, uint64_t& now, uint8_t k) {
  rt.home[leader]->apply(rt.at[leader], Command::ClientRequest(k, {k}), now += 10);
  rt.home[leader]->apply(rt.at[leader], Command::Tick(), now += 10);
  deliver_all(rt, wire, now);
  rt.home[leader]->apply(rt.at[leader], Command::Tick(), now += 150);
  deliver_all(rt, wire, now);
}

int main() {
  try {
    std::deque<Message> wire;
    BatchedRaft a(3, {1, 2, 3}, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY);
    a.rpc_tx = [&](const Message& m) { wire.push_back(m); };
    if (jg_set_self_slots(a.raw(), kSlots) != JG_OK) throw std::runtime_error("jg_set_self_slots");
    Route rt{{&a, &a, &a}, {0, 1, 2}};
    a.apply(0, Command::Timeout());  // node 1 campaigns and wins
    deliver_all(rt, wire, 0);
    CHECK(a.handle(0).is_leader());
    const uint64_t term = a.handle(0).current_term();
    uint64_t now = 0;
    for (uint8_t k = 1; k <= 3; k++) propose(rt, 0, wire, now, k);
    for (uint32_t g = 0; g < 3; g++) CHECK(a.handle(g).commit() == 3 && a.store(g).commit() == 3 && a.handle(g).fault() == 0);
    // the leader's instance moves to another engine of the same node (another GPU / process): state and store
    BatchedRaft b(1, {1, 2, 3}, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY);
    b.rpc_tx = [&](const Message& m) { wire.push_back(m); };
    BatchedRaft::GroupImage im = a.export_groups(0, 1);
    CHECK(im.header.n == 1 && im.header.n_replicas == 3 && im.header.record_bytes % 64 == 0 && im.stores.size() == 1);
    b.import_groups(std::move(im), 0);
    rt.home[0] = &b, rt.at[0] = 0;  // (instance 0 of `a` is no longer driven)
    RaftHandle h = b.handle(0);
    CHECK(h.is_leader() && h.current_term() == term && h.commit() == 3 && h.head() == 3 && h.fault() == 0);
    CHECK(b.store(0).commit() == 3 && b.store(0).has(3));
    // the cluster keeps committing: same leader, same term, no election
    for (uint8_t k = 4; k <= 6; k++) propose(rt, 0, wire, now, k);
    CHECK(h.is_leader() && h.current_term() == term && h.fault() == 0);
    CHECK(h.commit() == 6 && h.head() == 6 && b.store(0).commit() == 6 && b.store(0).has(6));
    for (uint32_t g = 1; g < 3; g++) {
      CHECK(a.handle(g).is_follower() && a.handle(g).current_term() == term && a.handle(g).fault() == 0);
      CHECK(a.handle(g).commit() == 6 && a.store(g).commit() == 6 && a.store(g).at(6).data == std::vector<uint8_t>{6});
    }
    // ... and through the timers: a long quiet stretch of heartbeats keeps the followers from campaigning
    for (int t = 0; t < 10; t++) {
      now += 150;
      b.apply(0, Command::Tick(), now);
      deliver_all(rt, wire, now);
      for (uint32_t g = 1; g < 3; g++) a.apply(g, Command::Tick(), now), deliver_all(rt, wire, now);
    }
    CHECK(h.is_leader() && h.current_term() == term);
    for (uint32_t g = 1; g < 3; g++) CHECK(a.handle(g).is_follower() && a.handle(g).current_term() == term);

    // a follower moves with a client request queued (no leader known yet: follower.rs:258-270): when it learns the
    // leader it forwards the request - with its proposal, which has moved with it - and the leader commits that payload
    std::deque<Message> wire2;
    BatchedRaft a2(3, {1, 2, 3}, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY);
    a2.rpc_tx = [&](const Message& m) { wire2.push_back(m); };
    if (jg_set_self_slots(a2.raw(), kSlots) != JG_OK) throw std::runtime_error("jg_set_self_slots");
    a2.apply(2, Command::ClientRequest(77, {7, 7, 7}), 0);
    CHECK(wire2.empty() && a2.handle(2).is_follower());
    BatchedRaft c2(1, {1, 2, 3}, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY);
    c2.rpc_tx = [&](const Message& m) { wire2.push_back(m); };
    BatchedRaft::GroupImage im2 = a2.export_groups(2, 1);
    CHECK(im2.queued.size() == 1 && im2.queued[0].size() == 1 && im2.proposals[0].count(77) == 1);
    c2.import_groups(std::move(im2), 0);
    Route rt2{{&a2, &a2, &c2}, {0, 1, 0}};  // node 3 now lives in c2
    uint64_t now2 = 0;
    a2.apply(0, Command::Timeout(), now2);  // node 1 campaigns and wins; its Heartbeat tells node 3 the leader
    deliver_all(rt2, wire2, now2);
    CHECK(a2.handle(0).is_leader());
    for (int t = 0; t < 3; t++) {  // the forwarded request is appended, replicated and committed
      a2.apply(0, Command::Tick(), now2 += 150);
      deliver_all(rt2, wire2, now2);
    }
    const BlockId head2 = a2.handle(0).head();
    CHECK(head2 >= 1 && a2.handle(0).commit() == head2 && c2.handle(0).commit() == head2 && c2.handle(0).fault() == 0);
    bool found = false;
    for (BlockId id = 1; id <= head2; id++)
      if (a2.store(0).has(id) && a2.store(0).at(id).data == std::vector<uint8_t>({7, 7, 7})) {
        found = true;
        CHECK((c2.store(0).has(id) && c2.store(0).at(id).data == std::vector<uint8_t>{7, 7, 7}));
      }
    CHECK(found);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("move groups ok");
  return 0;
}
