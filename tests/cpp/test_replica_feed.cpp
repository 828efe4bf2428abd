// The replication feed and its census through the C++ host mirror (BatchedRaft::watch_replicas / replication_census:
// jg_engine_watch_replicas / jg_engine_replication_census, ABI v15).  Three BatchedRafts - three brokers with the
// examples/multi-node ids 1, 2, 3 - host the same eight partitions; broker g % 3 campaigns for partition g and wins through
// the wire, clients append and every follower acknowledges: the leaders' feeds report whole in-sync sets.  Then broker 3's
// inbound traffic is withheld while clients keep appending: the feed of each of the other two reports slot 2 leaving the set
// of every partition it leads, and its census names slot 2 in out_of_sync.  Traffic resumes: the feeds report slot 2
// rejoining.  isr_nodes() turns a row's mask into the node ids Partition.isr holds.  Built and run by
// tests/test_cpp_replica_feed.py (-m gpu).
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

static const uint32_t kG = 8;       // partitions per broker
static const uint32_t kDown = 2;    // the broker (index; node id 3, member slot 2) whose inbound traffic is withheld
static const jg_isr_policy kPolicy = {2, 0};  // leaves above a lag of 2 blocks, rejoins caught up

// everything on the wire delivered to its addressees: node id i + 1 is broker i; what is addressed to a withheld broker is lost
static void deliver_all(BatchedRaft* b[3], std::deque<Message>& wire, uint64_t now, int withheld = -1) {
  int guard = 0;
  while (!wire.empty() && guard++ < 100000) {
    const Message m = wire.front();
    wire.pop_front();
    for (uint32_t dst = 0; dst < 3; dst++) {
      const NodeId id = dst + 1;
      if ((int)dst == withheld) continue;
      if ((m.to.kind == JG_TO_PEERS && id != m.from.peer) || (m.to.kind == JG_TO_PEER && m.to.peer == id))
        b[dst]->apply(m.group, m.command, now);
    }
  }
}

// one round: a client appends to every partition at its leader, the leaders tick, the wire drains
static void round_of_appends(BatchedRaft* b[3], std::deque<Message>& wire, uint64_t& now, uint64_t& request, int withheld = -1) {
  for (uint32_t g = 0; g < kG; g++) {
    b[g % 3]->apply(g, Command::ClientRequest(++request, {1, 2, 3}), now);
    deliver_all(b, wire, now, withheld);
  }
  now += 150;
  for (uint32_t g = 0; g < kG; g++) {
    b[g % 3]->apply(g, Command::Tick(), now);
    deliver_all(b, wire, now, withheld);
  }
}

int main() {
  try {
    std::deque<Message> wire;
    std::unique_ptr<BatchedRaft> own[3];
    BatchedRaft* b[3];
    for (uint32_t i = 0; i < 3; i++) {
      own[i].reset(new BatchedRaft(kG, {1, 2, 3}, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY));
      b[i] = own[i].get();
      const std::vector<uint8_t> slots(kG, (uint8_t)i);
      CHECK(jg_set_self_slots(b[i]->raw(), slots.data()) == JG_OK);
      b[i]->rpc_tx = [&wire](const Message& m) { wire.push_back(m); };
      // a fresh engine leads nothing: the feed is empty
      size_t total = 7;
      CHECK(b[i]->watch_replicas(kPolicy, 0, UINT32_MAX, SIZE_MAX, false, &total).empty() && total == 0);
      CHECK(b[i]->replication_census(2).leaders == 0);
    }
    uint64_t now = 0, request = 0;
    for (uint32_t g = 0; g < kG; g++) {
      b[g % 3]->apply(g, Command::Timeout(), now);
      deliver_all(b, wire, now);
      CHECK(b[g % 3]->handle(g).is_leader());
    }
    for (int r = 0; r < 3; r++) round_of_appends(b, wire, now, request);
    now += 150;
    for (uint32_t g = 0; g < kG; g++) {  // (one more tick: the last acknowledgements are in)
      b[g % 3]->apply(g, Command::Tick(), now);
      deliver_all(b, wire, now);
    }
    // every leader's feed: its partitions, whole sets (a peek first: the same rows, nothing advanced)
    uint32_t leads[3] = {0, 0, 0};
    for (uint32_t g = 0; g < kG; g++) leads[g % 3]++;
    for (uint32_t i = 0; i < 3; i++) {
      size_t total = 0;
      const std::vector<jg_isr_row> peek = b[i]->watch_replicas(kPolicy, 0, UINT32_MAX, 1, true, &total);
      CHECK(total == leads[i] && peek.size() == 1);
      const std::vector<jg_isr_row> rows = b[i]->watch_replicas(kPolicy, 0, UINT32_MAX, SIZE_MAX, false, &total);
      CHECK(total == leads[i] && rows.size() == leads[i]);
      if (!rows.empty() && !peek.empty()) CHECK(std::memcmp(&peek[0], &rows[0], sizeof(jg_isr_row)) == 0);
      for (const jg_isr_row& r : rows) {
        CHECK(r.group % 3 == i && r.isr == 7 && r.state == JG_ISR_LEADS && r.self_slot == i && r.worst_lag == 0 && r.head >= 3);
        CHECK((b[i]->isr_nodes(r.isr) == std::vector<int32_t>{1, 2, 3}));
      }
      CHECK(b[i]->watch_replicas(kPolicy).empty());
      const jg_repl_census c = b[i]->replication_census(2);
      CHECK(c.leaders == leads[i] && c.fully_replicated == leads[i] && c.under_replicated == 0 && c.below_quorum == 0);
      for (uint32_t k = 0; k < JG_MAX_REPLICAS; k++) CHECK(c.out_of_sync[k] == 0 && c.max_lag[k] == 0);
    }
    // broker 3 hears nothing any more; clients keep appending
    for (int r = 0; r < 4; r++) round_of_appends(b, wire, now, request, (int)kDown);
    for (uint32_t i = 0; i < 3; i++) {
      if (i == kDown) continue;
      size_t total = 0;
      const std::vector<jg_isr_row> rows = b[i]->watch_replicas(kPolicy, 0, UINT32_MAX, SIZE_MAX, false, &total);
      CHECK(total == leads[i] && rows.size() == leads[i]);  // ... for every partition it leads
      for (const jg_isr_row& r : rows) {
        CHECK(r.group % 3 == i && r.isr == (7u & ~(1u << kDown)) && r.state == (JG_ISR_LEADS | JG_ISR_UNDER) && r.worst_lag > kPolicy.leave_lag);
        CHECK((b[i]->isr_nodes(r.isr) == std::vector<int32_t>{1, 2}));
      }
      CHECK(b[i]->watch_replicas(kPolicy).empty());
      const jg_repl_census c = b[i]->replication_census(kPolicy.leave_lag);
      CHECK(c.leaders == leads[i] && c.under_replicated == leads[i] && c.fully_replicated == 0 && c.below_quorum == 0);
      CHECK(c.out_of_sync[kDown] == leads[i] && c.max_lag[kDown] > kPolicy.leave_lag && c.sum_lag[kDown] >= c.max_lag[kDown]);
      for (uint32_t k = 0; k < JG_MAX_REPLICAS; k++)
        if (k != kDown) CHECK(c.out_of_sync[k] == 0);
    }
    // traffic resumes: the leaders' ticks bring broker 3 up to date, the feeds report it rejoining
    std::vector<jg_isr_row> back[3];
    for (int r = 0; r < 12; r++) {
      now += 150;
      for (uint32_t g = 0; g < kG; g++) {
        b[g % 3]->apply(g, Command::Tick(), now);
        deliver_all(b, wire, now);
      }
      for (uint32_t i = 0; i < 3; i++) {
        if (i == kDown) continue;
        for (const jg_isr_row& row : b[i]->watch_replicas(kPolicy)) back[i].push_back(row);
      }
      if (back[0].size() >= leads[0] && back[1].size() >= leads[1]) break;
    }
    for (uint32_t i = 0; i < 3; i++) {
      if (i == kDown) continue;
      CHECK(back[i].size() == leads[i]);
      for (const jg_isr_row& r : back[i]) CHECK(r.group % 3 == i && r.isr == 7 && r.state == JG_ISR_LEADS && r.worst_lag <= kPolicy.join_lag);
      CHECK(b[i]->replication_census(kPolicy.leave_lag).fully_replicated == leads[i]);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("replica feed ok");
  return 0;
}
