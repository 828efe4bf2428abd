// The leadership feed and the census through the C++ host mirror (BatchedRaft::watch_leaders / census:
// jg_engine_watch_leaders / jg_engine_census, ABI v14).  Three BatchedRafts - three brokers with the examples/multi-node
// ids 1, 2, 3 - host the same eight partitions; broker g % 3 campaigns for partition g and wins through the wire.  Every
// broker's feed then names the same leader and term for each partition, exactly one broker reports SELF, the brokers'
// censuses add up, and a quiet feed reports nothing.  Then broker 3 deletes its replica of one partition: its feed says
// VACANT for that slot and nothing else.  Built and run by tests/test_cpp_leader_feed.py (-m gpu).
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

static const uint32_t kG = 8;  // partitions per broker
static const uint32_t kP = 5;  // the partition broker 3 deletes its replica of

// everything on the wire delivered to its addressees: node id i + 1 is broker i
static void deliver_all(BatchedRaft* b[3], std::deque<Message>& wire, uint64_t now) {
  int guard = 0;
  while (!wire.empty() && guard++ < 10000) {
    const Message m = wire.front();
    wire.pop_front();
    for (uint32_t dst = 0; dst < 3; dst++) {
      const NodeId id = dst + 1;
      if ((m.to.kind == JG_TO_PEERS && id != m.from.peer) || (m.to.kind == JG_TO_PEER && m.to.peer == id))
        b[dst]->apply(m.group, m.command, now);
    }
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
      // a fresh hosted engine reports every slot once: followers at term 0 that know no leader
      size_t total = 0;
      const std::vector<jg_leader_row> rows = b[i]->watch_leaders(0, UINT32_MAX, SIZE_MAX, false, &total);
      CHECK(total == kG && rows.size() == kG);
      for (uint32_t g = 0; g < rows.size(); g++)
        CHECK(rows[g].group == g && rows[g].role == JG_ROLE_FOLLOWER && rows[g].term == 0 && rows[g].state == 0 && rows[g].leader_id == 0 &&
              rows[g].self_slot == i && rows[g].fault == 0 && rows[g].reserved == 0);
      CHECK(b[i]->watch_leaders().empty());
      const jg_census c = b[i]->census();
      CHECK(c.hosted == kG && c.followers == kG && c.leaderless == kG && c.leaders == 0 && c.max_term == 0);
    }
    // broker g % 3 campaigns for partition g and wins; its first Tick's Heartbeat tells the followers who leads
    uint64_t now = 0;
    for (uint32_t g = 0; g < kG; g++) {
      b[g % 3]->apply(g, Command::Timeout(), now);
      deliver_all(b, wire, now);
      CHECK(b[g % 3]->handle(g).is_leader());
    }
    now += 150;
    for (uint32_t g = 0; g < kG; g++) {
      b[g % 3]->apply(g, Command::Tick(), now);
      deliver_all(b, wire, now);
    }
    // a peek first: the same rows, nothing advanced
    std::vector<jg_leader_row> feed[3];
    jg_census cs[3];
    for (uint32_t i = 0; i < 3; i++) {
      size_t total = 0;
      const std::vector<jg_leader_row> peek = b[i]->watch_leaders(0, UINT32_MAX, 3, true, &total);
      CHECK(total == kG && peek.size() == 3);
      feed[i] = b[i]->watch_leaders(0, UINT32_MAX, SIZE_MAX, false, &total);
      CHECK(total == kG && feed[i].size() == kG);
      for (size_t k = 0; k < peek.size() && k < feed[i].size(); k++) CHECK(std::memcmp(&peek[k], &feed[i][k], sizeof(jg_leader_row)) == 0);
      cs[i] = b[i]->census();
    }
    for (uint32_t g = 0; g < kG && feed[0].size() == kG && feed[1].size() == kG && feed[2].size() == kG; g++) {
      uint32_t selfs = 0;
      for (uint32_t i = 0; i < 3; i++) {
        const jg_leader_row& r = feed[i][g];
        CHECK(r.group == g && r.leader_id == g % 3 + 1 && r.term == feed[0][g].term && r.term >= 1 && (r.state & JG_LEAD_KNOWN));
        CHECK(!(r.state & (JG_LEAD_VACANT | JG_LEAD_FAULTED)) && r.fault == 0);
        CHECK(((r.state & JG_LEAD_SELF) != 0) == (i == g % 3) && (r.role == JG_ROLE_LEADER) == (i == g % 3));
        CHECK(r.term == b[i]->handle(g).current_term());
        selfs += (r.state & JG_LEAD_SELF) ? 1 : 0;
      }
      CHECK(selfs == 1);
    }
    uint64_t leaders = 0;
    for (uint32_t i = 0; i < 3; i++) {
      leaders += cs[i].leaders;
      CHECK(cs[i].hosted == kG && cs[i].vacant == 0 && cs[i].leaderless == 0 && cs[i].candidates == 0 && cs[i].led_by_other == 0);
      CHECK(cs[i].leaders + cs[i].followers == kG && cs[i].faulted_reference + cs[i].faulted_engine == 0);
      for (uint32_t k = 0; k < JG_MAX_REPLICAS; k++) CHECK(cs[i].led_by[k] == cs[0].led_by[k]);
      CHECK(cs[i].led_by[0] == 3 && cs[i].led_by[1] == 3 && cs[i].led_by[2] == 2 && cs[i].max_term == feed[0][0].term);
    }
    CHECK(leaders == kG);
    // steady state: heartbeats change nobody's view - the feed is quiet
    now += 150;
    for (uint32_t g = 0; g < kG; g++) {
      b[g % 3]->apply(g, Command::Tick(), now);
      deliver_all(b, wire, now);
    }
    for (uint32_t i = 0; i < 3; i++) CHECK(b[i]->watch_leaders().empty());
    // broker 3 deletes its replica of partition kP (which it leads): its feed says VACANT, the others' nothing
    b[2]->close_groups({kP});
    size_t total = 0;
    const std::vector<jg_leader_row> gone = b[2]->watch_leaders(0, UINT32_MAX, SIZE_MAX, false, &total);
    CHECK(total == 1 && gone.size() == 1);
    if (gone.size() == 1)
      CHECK(gone[0].group == kP && gone[0].state == JG_LEAD_VACANT && gone[0].fault == JG_FAULT_VACANT && gone[0].term == 0 &&
            gone[0].leader_id == 0 && gone[0].role == 0 && gone[0].self_slot == 2);
    CHECK(b[0]->watch_leaders().empty() && b[1]->watch_leaders().empty() && b[2]->watch_leaders().empty());
    const jg_census c3 = b[2]->census();
    CHECK(c3.vacant == 1 && c3.hosted == kG - 1 && c3.leaders == cs[2].leaders - 1);
    CHECK(b[2]->census(kP, 1).vacant == 1 && b[2]->census(kP, 1).hosted == 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("leader feed ok");
  return 0;
}
