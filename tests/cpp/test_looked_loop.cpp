// Point queries of a loop with two ticks in flight, through the C++ host mirror (BatchedEventLoop::lookup_async over
// BatchedRaft::step_node_looked / node_lookup: jg_step_node_looked / jg_node_lookup_view, ABI v25).  ONE pipelined event loop
// with in_flight = 2 over a few thousand partitions this node leads, clients appending all the time: every tick asks for the
// state of a random list of partitions (some ticks twice, with and without the progress heads: requests that agree share a
// step), and a sink receives the rows when the outputs of the tick that carried the request are consumed.  A few partitions
// follow and learn their leader from a Heartbeat halfway: a row of the general path, so that tick's lookup comes back redone.
// Every sink is called exactly once, in request order, with one row per entry in the order asked, and no row is older -
// term, head, commit - than what the loop's own sinks had shown of that partition when the request was made.  Afterwards a
// last request equals the synchronous BatchedRaft::lookup.  Built and run by tests/test_cpp_looked_loop.py (-m gpu).
#include <cstdio>
#include <cstring>
#include <random>

#include "../../josefine_amd/host/formats.hpp"  // (includes raft_handle.hpp)

using namespace josefine;

static int g_failed = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      if (g_failed < 20) std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_failed++;                                                                    \
    }                                                                                \
  } while (0)

int main() {
  const uint32_t G = 3000 + 37, T = 24, R = 3;
  std::vector<NodeId> ids{1, 2, 3};
  BatchedRaft raft(G, ids, 0, 5, JG_CFG_SEPARATE_COMMIT_KEY);
  BatchedEventLoop loop(raft, G);
  loop.halves = JG_NODE_LEADER_HALF;
  loop.pipelined = true, loop.in_flight = 2;
  auto follows = [](uint32_t g) { return g % 97 == 5; };
  {  // this node wins the election of every other partition the reference's way: Timeout, then a granted vote
    RowQueue q;
    for (uint32_t g = 0; g < G; g++)
      if (!follows(g)) q.push(g, JG_CMD_TIMEOUT);
    raft.submit_rows(q.view());
    raft.step(0);
    q.clear();
    for (uint32_t g = 0; g < G; g++)
      if (!follows(g)) q.push(g, JG_CMD_VOTE_RESPONSE, ids[1], 1, 0, 0, 1);
    raft.submit_rows(q.view());
    raft.step(0);
  }
  // what the loop's own sinks have shown of a partition: where it stood before the first tick, then every block fsm_tx
  // reported appended (Notify: the head is there at least) and applied (the commit is there at least)
  std::vector<uint64_t> term(G), head(G), commit(G);
  {
    const BatchedRaft::GroupStates s0 = raft.lookup(0u, G);
    for (uint32_t g = 0; g < G; g++) term[g] = s0.rows[g].term, head[g] = s0.rows[g].head, commit[g] = s0.rows[g].commit;
  }
  uint64_t general = 0, notified = 0;
  raft.fsm_rows_tx = [&](const jg_fsm_row* rows, size_t n) {
    for (size_t i = 0; i < n; i++) {
      const jg_fsm_row& r = rows[i];
      if (r.kind == JG_FSM_NOTIFY) head[r.group] = std::max(head[r.group], r.a), notified++;
      if (r.kind == JG_FSM_APPLY_LEADER) commit[r.group] = std::max(commit[r.group], r.b);
    }
  };
  raft.msg_rows_tx = [&](const jg_msg_row*, size_t) {};
  raft.columns_tx = [&](const jg_node_outbox& o) { general += o.rows_general; };

  struct Ask {
    std::vector<uint32_t> list;
    std::vector<uint64_t> term, head, commit;  // as the sinks had shown them when the request was made
    bool progress;
  };
  std::vector<Ask> asks;
  size_t answered = 0;
  uint64_t redone_answers = 0, rows_seen = 0, moved = 0;
  std::mt19937 rng(7);
  auto ask = [&](size_t n, bool progress) {
    Ask a;
    a.progress = progress;
    for (size_t i = 0; i < n; i++) {
      const uint32_t g = rng() % G;
      a.list.push_back(g), a.term.push_back(term[g]), a.head.push_back(head[g]), a.commit.push_back(commit[g]);
    }
    const size_t seq = asks.size();
    asks.push_back(a);
    loop.lookup_async(a.list, progress, [&, seq](const BatchedRaft::GroupStates& s, bool redone) {
      CHECK(seq == answered);  // exactly once, in request order
      answered++;
      redone_answers += redone;
      const Ask& q = asks[seq];
      CHECK(s.rows.size() == q.list.size());
      CHECK(s.match.size() == (q.progress ? q.list.size() * R : 0));
      for (size_t i = 0; i < q.list.size() && i < s.rows.size(); i++) {
        const jg_group_state& r = s.rows[i];
        CHECK(r.group == q.list[i]);
        CHECK(r.term >= q.term[i] && r.head >= q.head[i] && r.commit >= q.commit[i]);
        CHECK(r.commit <= r.head);
        moved += r.head > q.head[i];
      }
      rows_seen += s.rows.size();
    });
  };

  std::vector<uint64_t> appended(G, 0);
  for (uint32_t t = 0; t < T; t++) {
    RowQueue in;
    for (uint32_t g = 0; g < G; g++) {
      if (follows(g)) {  // its leader's Heartbeat: the follower learns who leads (the general path: the follower half does not run)
        if (t == T / 2) in.push(g, JG_CMD_HEARTBEAT, ids[2], 1, 0, 0, 0);
        continue;
      }
      if ((g + t) % 3 == 0) continue;  // a quiet partition this tick
      if (appended[g]) in.push(g, JG_CMD_APPEND_RESPONSE, ids[1], 1, appended[g], 0, 1);  // the member acknowledges what it has
      if ((g + 2 * t) % 5) in.push(g, JG_CMD_CLIENT_REQUEST, 0, 0, (uint64_t)t * G + g + 1), appended[g]++;
    }
    loop.tcp_rx_rows(in.view());
    ask(t == 3 ? 0 : 1 + rng() % 700, t % 2 == 1);
    if (t % 4 == 1) ask(1 + rng() % 300, true);    // agrees with the tick's first request: the same step
    if (t % 4 == 2) ask(1 + rng() % 300, true);    // does not: the next tick's step, in front of that tick's own
    loop.run_until((uint64_t)t * BatchedEventLoop::TICK_MS);
  }
  for (uint32_t t = T; t < T + 4; t++) loop.run_until((uint64_t)t * BatchedEventLoop::TICK_MS);
  loop.flush();
  CHECK(answered == asks.size());
  CHECK(redone_answers >= 1 && redone_answers < answered);
  CHECK(general > 0 && notified > G && rows_seen > 0 && moved > 0);
  // nothing is outstanding: a last request, carried by one more tick, is the synchronous lookup's answer
  {
    std::vector<uint32_t> list;
    for (uint32_t i = 0; i < 500; i++) list.push_back(rng() % G);
    BatchedRaft::GroupStates got;
    size_t calls = 0;
    loop.lookup_async(list, true, [&](const BatchedRaft::GroupStates& s, bool) { got = s, calls++; });
    loop.run_until((uint64_t)(T + 4) * BatchedEventLoop::TICK_MS);
    CHECK(calls == 0);  // (two ticks in flight: the tick is still open)
    loop.flush();
    CHECK(calls == 1);
    const BatchedRaft::GroupStates want = raft.lookup(list.data(), list.size(), true);
    CHECK(got.rows.size() == want.rows.size() && got.match == want.match);
    CHECK(got.rows.size() == want.rows.size() && !std::memcmp(got.rows.data(), want.rows.data(), want.rows.size() * sizeof(jg_group_state)));
    // ... and on a loop below two in flight no step is kept: the synchronous call answers at the next step boundary
    loop.in_flight = 1;
    calls = 0;
    loop.lookup_async(list, true, [&](const BatchedRaft::GroupStates& s, bool redone) {
      got = s, calls++;
      CHECK(!redone);
    });
    loop.run_until((uint64_t)(T + 5) * BatchedEventLoop::TICK_MS);
    CHECK(calls == 1);
    CHECK(got.rows.size() == want.rows.size() && !std::memcmp(got.rows.data(), want.rows.data(), want.rows.size() * sizeof(jg_group_state)));
    loop.flush();
  }
  if (g_failed) {
    std::fprintf(stderr, "%d checks failed (asked %zu, answered %zu, redone %llu)\n", g_failed, asks.size(), answered,
                 (unsigned long long)redone_answers);
    return 1;
  }
  std::printf("looked loop ok: %zu requests (%llu redone), %llu rows\n", answered, (unsigned long long)redone_answers,
              (unsigned long long)rows_seen);
  return 0;
}
