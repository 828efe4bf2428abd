// Time-based in-sync sets through the C++ host mirror (BatchedRaft::watch_replicas_timed: jg_engine_watch_replicas_timed,
// ABI v19).  Three BatchedRafts - three brokers with the examples/multi-node ids 1, 2, 3 - host the same eight partitions;
// broker g % 3 campaigns for partition g and wins through the wire, clients append and every follower acknowledges: the
// leaders' feeds report whole in-sync sets.  Then broker 3's inbound traffic is withheld while clients keep appending.  Under
// the time rule the leaders' feeds say nothing while slot 2 has been behind for less than kMaxBehind ms of the caller's clock
// - however many blocks that is - and report it leaving with the first sample past that; a peek before says the same and
// advances nothing.  Traffic resumes: the feeds report slot 2 rejoining once it has caught up.  Built and run by
// tests/test_cpp_isr_clock.py (-m gpu).
#include <cstdio>
#include <cstring>
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

static const uint32_t kG = 8;            // partitions per broker
static const uint32_t kDown = 2;         // the broker (index; node id 3, member slot 2) whose inbound traffic is withheld
static const uint64_t kMaxBehind = 1000;  // replica.lag.time.max.ms

static jg_isr_clock at(uint64_t now_ms) { return jg_isr_clock{now_ms, kMaxBehind, 0, 0}; }

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

static void tick_all(BatchedRaft* b[3], std::deque<Message>& wire, uint64_t& now, int withheld = -1) {
  now += 150;
  for (uint32_t g = 0; g < kG; g++) {
    b[g % 3]->apply(g, Command::Tick(), now);
    deliver_all(b, wire, now, withheld);
  }
}

// one round: a client appends to every partition at its leader, the leaders tick, the wire drains
static void round_of_appends(BatchedRaft* b[3], std::deque<Message>& wire, uint64_t& now, uint64_t& request, int withheld = -1) {
  for (uint32_t g = 0; g < kG; g++) {
    b[g % 3]->apply(g, Command::ClientRequest(++request, {1, 2, 3}), now);
    deliver_all(b, wire, now, withheld);
  }
  tick_all(b, wire, now, withheld);
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
      size_t total = 7;  // a fresh engine leads nothing: the feed is empty
      CHECK(b[i]->watch_replicas_timed(at(0), 0, UINT32_MAX, SIZE_MAX, false, &total).empty() && total == 0);
    }
    uint64_t now = 0, request = 0;
    for (uint32_t g = 0; g < kG; g++) {
      b[g % 3]->apply(g, Command::Timeout(), now);
      deliver_all(b, wire, now);
      CHECK(b[g % 3]->handle(g).is_leader());
    }
    for (int r = 0; r < 3; r++) round_of_appends(b, wire, now, request);
    tick_all(b, wire, now);  // (one more tick: the last acknowledgements are in)
    uint32_t leads[3] = {0, 0, 0};
    for (uint32_t g = 0; g < kG; g++) leads[g % 3]++;
    for (uint32_t i = 0; i < 3; i++) {  // whole sets (a peek first: the same rows, nothing advanced)
      size_t total = 0;
      const std::vector<jg_isr_row> peek = b[i]->watch_replicas_timed(at(now), 0, UINT32_MAX, 1, true, &total);
      CHECK(total == leads[i] && peek.size() == 1);
      const std::vector<jg_isr_row> rows = b[i]->watch_replicas_timed(at(now), 0, UINT32_MAX, SIZE_MAX, false, &total);
      CHECK(total == leads[i] && rows.size() == leads[i]);
      if (!rows.empty() && !peek.empty()) CHECK(std::memcmp(&peek[0], &rows[0], sizeof(jg_isr_row)) == 0);
      for (const jg_isr_row& r : rows) {
        CHECK(r.group % 3 == i && r.isr == 7 && r.state == JG_ISR_LEADS && r.self_slot == i && r.worst_lag == 0 && r.head >= 3);
        CHECK((b[i]->isr_nodes(r.isr) == std::vector<int32_t>{1, 2, 3}));
      }
      CHECK(b[i]->watch_replicas_timed(at(now)).empty());
    }
    // broker 3 hears nothing any more; clients keep appending.  The first sample that sees it behind starts its clocks
    round_of_appends(b, wire, now, request, (int)kDown);
    tick_all(b, wire, now, (int)kDown);
    const uint64_t seen_behind = now;
    for (uint32_t i = 0; i < 3; i++)
      if (i != kDown) CHECK(b[i]->watch_replicas_timed(at(seen_behind)).empty());
    // ... many blocks behind, and still in: nothing is reported inside the window
    for (int r = 0; r < 4; r++) round_of_appends(b, wire, now, request, (int)kDown);
    tick_all(b, wire, now, (int)kDown);
    CHECK(now - seen_behind <= kMaxBehind);
    for (uint32_t i = 0; i < 3; i++) {
      if (i == kDown) continue;
      CHECK(b[i]->watch_replicas_timed(at(now)).empty());
      CHECK(b[i]->replication_census(2).out_of_sync[kDown] == leads[i]);  // (the lag rule would have dropped it by now)
      // a peek past the window sees it leave; the watch at the window's last millisecond does not
      size_t total = 0;
      CHECK(b[i]->watch_replicas_timed(at(seen_behind + kMaxBehind + 1), 0, UINT32_MAX, SIZE_MAX, true, &total).size() == leads[i]);
      CHECK(b[i]->watch_replicas_timed(at(seen_behind + kMaxBehind)).empty());
    }
    for (uint32_t i = 0; i < 3; i++) {
      if (i == kDown) continue;
      size_t total = 0;
      const std::vector<jg_isr_row> rows = b[i]->watch_replicas_timed(at(seen_behind + kMaxBehind + 1), 0, UINT32_MAX, SIZE_MAX, false, &total);
      CHECK(total == leads[i] && rows.size() == leads[i]);  // ... for every partition it leads
      for (const jg_isr_row& r : rows) {
        CHECK(r.group % 3 == i && r.isr == (7u & ~(1u << kDown)) && r.state == (JG_ISR_LEADS | JG_ISR_UNDER) && r.worst_lag >= 5);
        CHECK((b[i]->isr_nodes(r.isr) == std::vector<int32_t>{1, 2}));
      }
      CHECK(b[i]->watch_replicas_timed(at(seen_behind + kMaxBehind + 1)).empty());
    }
    // traffic resumes: the leaders' ticks bring broker 3 up to date, the feeds report it rejoining
    now = seen_behind + kMaxBehind + 1;
    std::vector<jg_isr_row> back[3];
    for (int r = 0; r < 12; r++) {
      tick_all(b, wire, now);
      for (uint32_t i = 0; i < 3; i++) {
        if (i == kDown) continue;
        for (const jg_isr_row& row : b[i]->watch_replicas_timed(at(now))) back[i].push_back(row);
      }
      if (back[0].size() >= leads[0] && back[1].size() >= leads[1]) break;
    }
    for (uint32_t i = 0; i < 3; i++) {
      if (i == kDown) continue;
      CHECK(back[i].size() == leads[i]);
      for (const jg_isr_row& r : back[i]) CHECK(r.group % 3 == i && r.isr == 7 && r.state == JG_ISR_LEADS && r.worst_lag == 0);
    }
    // refusals: the clock of the caller is never UINT64_MAX; join_lag <= caught_lag
    for (const jg_isr_clock& bad : {jg_isr_clock{UINT64_MAX, 1, 0, 0}, jg_isr_clock{5, 1, 1, 2}}) {
      bool refused = false;
      try {
        b[0]->watch_replicas_timed(bad);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("isr clock ok");
  return 0;
}
