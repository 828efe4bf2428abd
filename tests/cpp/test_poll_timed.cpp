// Poll under the time rule through the C++ host mirror (BatchedRaft::poll with PollRequest::timed: jg_poll.clock, ABI v20)
// against the separate C++ calls on a TWIN.  Two worlds of three brokers each (ids 1, 2, 3; broker g % 3 leads partition g)
// exchange the same messages; broker 3's inbound traffic is withheld while clients keep appending.  At every sample - whole
// sets, the sample that starts the clocks, inside the window, its last millisecond, expiry, the rejoin - each broker of one
// world is asked with watch_leaders, watch_replicas_timed and watch_commits, its twin in the other with ONE poll carrying the
// clock (halfway the worlds swap); a timed peek past the window is compared first and moves nothing.  Everything returned
// is equal byte for byte, and the members leave at the sample the clock says.  Built and run by
// tests/test_cpp_poll_timed.py (-m gpu).
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
static const int kDown = 2;              // the broker (index; node id 3, member slot 2) whose inbound traffic is withheld
static const uint64_t kMaxBehind = 1000;  // replica.lag.time.max.ms

// three brokers and the wire between them (tests/cpp/test_isr_clock.cpp)
struct World {
  std::deque<Message> wire;
  std::unique_ptr<BatchedRaft> b[3];
  uint64_t now = 0, request = 0;
  World() {
    for (uint32_t i = 0; i < 3; i++) {
      b[i].reset(new BatchedRaft(kG, {1, 2, 3}, 0, 0, JG_CFG_SEPARATE_COMMIT_KEY));
      const std::vector<uint8_t> slots(kG, (uint8_t)i);
      CHECK(jg_set_self_slots(b[i]->raw(), slots.data()) == JG_OK);
      b[i]->rpc_tx = [this](const Message& m) { wire.push_back(m); };
    }
    for (uint32_t g = 0; g < kG; g++) {
      b[g % 3]->apply(g, Command::Timeout(), now);
      deliver();
      CHECK(b[g % 3]->handle(g).is_leader());
    }
  }
  void deliver(int withheld = -1) {
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
  void tick(int withheld = -1) {
    now += 150;
    for (uint32_t g = 0; g < kG; g++) {
      b[g % 3]->apply(g, Command::Tick(), now);
      deliver(withheld);
    }
  }
  void appends(int withheld = -1) {
    for (uint32_t g = 0; g < kG; g++) {
      b[g % 3]->apply(g, Command::ClientRequest(++request, {1, 2, 3}), now);
      deliver(withheld);
    }
    tick(withheld);
  }
};

template <class Row>
static bool same_rows(const std::vector<Row>& a, const std::vector<Row>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(Row)) == 0);
}

static BatchedRaft::PollRequest request(uint64_t now_ms, bool peek = false, size_t replicas_limit = SIZE_MAX) {
  BatchedRaft::PollRequest q;  // (the three feeds)
  q.timed = true;
  q.clock = jg_isr_clock{now_ms, kMaxBehind, 0, 0};
  q.policy = jg_isr_policy{1, 2};  // (beside a clock the policy is not looked at: this one the lag rule refuses)
  q.leaders_peek = q.replicas_peek = q.commits_peek = peek;
  q.replicas_limit = replicas_limit;
  return q;
}

// the separate calls of one request, as a PollResult
static BatchedRaft::PollResult separate(BatchedRaft& e, const BatchedRaft::PollRequest& q) {
  BatchedRaft::PollResult r;
  r.leaders = e.watch_leaders(q.g0, q.n, q.leaders_limit, q.leaders_peek, &r.leaders_total);
  r.replicas = e.watch_replicas_timed(q.clock, q.g0, q.n, q.replicas_limit, q.replicas_peek, &r.replicas_total);
  r.commits = e.watch_commits(q.g0, q.n, q.commits_limit, q.commits_peek, q.commits_only, &r.commits_total, &r.backlog);
  return r;
}

// broker i of both worlds at one sample, one asked each way: the replicas rows
static std::vector<jg_isr_row> sample(World& x, World& y, uint32_t i, const BatchedRaft::PollRequest& q, bool swap) {
  BatchedRaft &sep = swap ? *y.b[i] : *x.b[i], &pol = swap ? *x.b[i] : *y.b[i];
  const BatchedRaft::PollResult s = separate(sep, q), p = pol.poll(q);
  CHECK(same_rows(s.leaders, p.leaders) && s.leaders_total == p.leaders_total);
  CHECK(same_rows(s.replicas, p.replicas) && s.replicas_total == p.replicas_total);
  CHECK(same_rows(s.commits, p.commits) && s.commits_total == p.commits_total);
  CHECK(std::memcmp(&s.backlog, &p.backlog, sizeof s.backlog) == 0);
  return p.replicas;
}

int main() {
  try {
    World x, y;
    uint32_t leads[3] = {0, 0, 0};
    for (uint32_t g = 0; g < kG; g++) leads[g % 3]++;
    for (World* w : {&x, &y}) {
      for (int r = 0; r < 3; r++) w->appends();
      w->tick();  // (one more tick: the last acknowledgements are in)
    }
    for (uint32_t i = 0; i < 3; i++) {  // whole sets
      const std::vector<jg_isr_row> rows = sample(x, y, i, request(x.now), false);
      CHECK(rows.size() == leads[i]);
      for (const jg_isr_row& r : rows) CHECK(r.isr == 7 && r.state == JG_ISR_LEADS);
      CHECK(sample(x, y, i, request(x.now), false).empty());
    }
    // broker 3 hears nothing any more; clients keep appending.  The first sample that sees it behind starts its clocks -
    // behind a limit of 0 too
    for (World* w : {&x, &y}) {
      w->appends(kDown);
      w->tick(kDown);
    }
    const uint64_t start = x.now;
    CHECK(y.now == start);
    for (uint32_t i = 0; i < 3; i++) CHECK(sample(x, y, i, request(start, false, i == 0 ? 0 : SIZE_MAX), false).empty());
    // inside the window: many blocks behind, and still in; a peek past the window sees it leave and moves nothing
    for (World* w : {&x, &y}) {
      for (int r = 0; r < 4; r++) w->appends(kDown);
    }
    CHECK(x.now - start <= kMaxBehind);
    for (uint32_t i = 0; i < 3; i++) {
      CHECK(sample(x, y, i, request(x.now), true).empty());
      const size_t leaving = sample(x, y, i, request(start + kMaxBehind + 1, true), true).size();
      if (i != (uint32_t)kDown) CHECK(leaving == leads[i]);  // (the withheld broker hears no acknowledgement either: only compared)
      CHECK(sample(x, y, i, request(start + kMaxBehind), true).empty());  // the last millisecond of the window
    }
    // expiry, at the sample the clock says
    for (uint32_t i = 0; i < 3; i++) {
      const std::vector<jg_isr_row> rows = sample(x, y, i, request(start + kMaxBehind + 1), true);
      if (i == (uint32_t)kDown) continue;
      CHECK(rows.size() == leads[i]);
      for (const jg_isr_row& r : rows) CHECK(r.isr == (7u & ~(1u << kDown)) && r.state == (JG_ISR_LEADS | JG_ISR_UNDER));
      CHECK(sample(x, y, i, request(start + kMaxBehind + 1), true).empty());
    }
    // traffic resumes: the feeds report broker 3 rejoining once it has caught up
    size_t back[3] = {0, 0, 0};
    for (World* w : {&x, &y}) w->now = start + kMaxBehind + 1;
    for (int r = 0; r < 12; r++) {
      for (World* w : {&x, &y}) w->tick();
      for (uint32_t i = 0; i < 3; i++)
        for (const jg_isr_row& row : sample(x, y, i, request(x.now), r % 2 == 0)) back[i] += row.isr == 7 ? 1 : 0;
      if (back[0] >= leads[0] && back[1] >= leads[1]) break;
    }
    CHECK(back[0] == leads[0] && back[1] == leads[1]);
    // the clock's own refusals, through the poll
    for (const jg_isr_clock& bad : {jg_isr_clock{UINT64_MAX, 1, 0, 0}, jg_isr_clock{5, 1, 1, 2}}) {
      BatchedRaft::PollRequest q = request(5);
      q.clock = bad;
      bool refused = false;
      try {
        x.b[0]->poll(q);
      } catch (const std::exception&) {
        refused = true;
      }
      CHECK(refused);
      q.want = JG_POLL_LEADERS;  // (the clock of a replicas part that is not wanted is not looked at)
      CHECK(x.b[0]->poll(q).leaders_total == 0);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("poll timed ok");
  return 0;
}
