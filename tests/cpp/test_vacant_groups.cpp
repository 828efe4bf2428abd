// Partitions created and deleted at runtime through the C++ host mirror: three BatchedRafts - three brokers with the
// examples/multi-node ids 1, 2, 3 - start with every slot vacant (JG_CFG_START_VACANT), as a broker that sizes its engine
// before it knows its partitions.  LeaderAndIsr then creates one partition on all three (BatchedRaft::open_groups:
// jg_engine_open_groups, ABI v13), which elects a leader and commits a request.  Then broker 3 deletes its replica
// (close_groups): its slot emits nothing more, whatever reaches it, while brokers 1 and 2 keep committing.  Built and run
// by tests/test_cpp_vacant_groups.py (-m gpu).
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

static const uint32_t kG = 8;  // slots per broker
static const uint32_t kP = 5;  // the slot the partition is opened in

// everything on the wire delivered to its addressees: node id i + 1 is broker i
static void deliver_all(BatchedRaft* b[3], std::deque<Message>& wire, uint64_t now) {
  int guard = 0;
  while (!wire.empty() && guard++ < 1000) {
    const Message m = wire.front();
    wire.pop_front();
    for (uint32_t dst = 0; dst < 3; dst++) {
      const NodeId id = dst + 1;
      if ((m.to.kind == JG_TO_PEERS && id != m.from.peer) || (m.to.kind == JG_TO_PEER && m.to.peer == id))
        b[dst]->apply(m.group, m.command, now);
    }
  }
}

static void propose(BatchedRaft* b[3], uint32_t leader, std::deque<Message>& wire, uint64_t& now, uint8_t k) {
  b[leader]->apply(kP, Command::ClientRequest(k, {k}), now += 10);
  b[leader]->apply(kP, Command::Tick(), now += 10);
  deliver_all(b, wire, now);
  b[leader]->apply(kP, Command::Tick(), now += 150);
  deliver_all(b, wire, now);
}

int main() {
  try {
    std::deque<Message> wire;
    size_t sent[3] = {0, 0, 0};
    std::unique_ptr<BatchedRaft> own[3];
    BatchedRaft* b[3];
    for (uint32_t i = 0; i < 3; i++) {
      own[i].reset(new BatchedRaft(kG, {1, 2, 3}, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY, {}, /*start_vacant=*/true));
      b[i] = own[i].get();
      b[i]->rpc_tx = [&wire, &sent, i](const Message& m) {
        wire.push_back(m);
        sent[i]++;
      };
      CHECK(b[i]->vacant_groups().size() == kG && b[i]->hosted_groups().empty());
      CHECK(b[i]->handle(kP).fault() == JG_FAULT_VACANT);
    }
    // rows for a partition nobody hosts yet are ignored: no message, no fault, no revival
    for (uint32_t i = 0; i < 3; i++) {
      b[i]->apply(kP, Command::Timeout(), 0);
      Command re;
      re.kind = JG_CMD_RECREATE;
      b[i]->apply(kP, re, 0);
      CHECK(b[i]->handle(kP).fault() == JG_FAULT_VACANT);
    }
    CHECK(wire.empty());
    // LeaderAndIsr: the partition is created on all three brokers, each in its own replica slot
    for (uint32_t i = 0; i < 3; i++) {
      const std::vector<uint8_t> slot{(uint8_t)i};
      b[i]->open_groups({kP}, 0, &slot);
      CHECK(b[i]->hosted_groups() == std::vector<uint32_t>{kP} && b[i]->vacant_groups().size() == kG - 1);
      CHECK(b[i]->handle(kP).is_follower() && b[i]->handle(kP).fault() == 0 && b[i]->store(kP).has(0));
    }
    b[0]->apply(kP, Command::Timeout(), 0);  // broker 1 campaigns and wins
    deliver_all(b, wire, 0);
    CHECK(b[0]->handle(kP).is_leader());
    const uint64_t term = b[0]->handle(kP).current_term();
    uint64_t now = 0;
    for (uint8_t k = 1; k <= 2; k++) propose(b, 0, wire, now, k);
    for (uint32_t i = 0; i < 3; i++) CHECK(b[i]->handle(kP).commit() == 2 && b[i]->store(kP).commit() == 2);
    CHECK(b[2]->store(kP).at(2).data == std::vector<uint8_t>{2});
    // broker 3 deletes its replica: vacant again, its store dropped
    b[2]->close_groups({kP});
    CHECK(b[2]->handle(kP).fault() == JG_FAULT_VACANT && b[2]->vacant_groups().size() == kG);
    CHECK(b[2]->handle(kP).commit() == 0 && b[2]->handle(kP).current_term() == 0);
    const size_t sent3 = sent[2];
    // the other two keep committing (a quorum of 3); broker 3's slot hears everything and says nothing, through the timers
    for (uint8_t k = 3; k <= 5; k++) propose(b, 0, wire, now, k);
    for (int t = 0; t < 10; t++) {
      now += 400;
      for (uint32_t i = 0; i < 3; i++) b[i]->apply(kP, Command::Tick(), now);
      deliver_all(b, wire, now);
    }
    CHECK(sent[2] == sent3);
    CHECK(b[2]->handle(kP).fault() == JG_FAULT_VACANT && b[2]->handle(kP).commit() == 0);
    CHECK(b[0]->handle(kP).is_leader() && b[0]->handle(kP).current_term() == term);
    for (uint32_t i = 0; i < 2; i++) {
      CHECK(b[i]->handle(kP).commit() == 5 && b[i]->store(kP).commit() == 5 && b[i]->handle(kP).fault() == 0);
      CHECK(b[i]->store(kP).at(5).data == std::vector<uint8_t>{5});
    }
    CHECK(b[1]->handle(kP).is_follower() && b[1]->handle(kP).current_term() == term);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("vacant groups ok");
  return 0;
}
