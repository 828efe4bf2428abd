// The completion feed of a loop with two ticks in flight, through the C++ host mirror (BatchedEventLoop::set_completions over
// BatchedRaft::step_node_awaited / node_completions: jg_step_node_awaited / jg_node_await_view, ABI v23).  ONE pipelined event
// loop with in_flight = 2 over a few thousand partitions this node leads: every Notify row a tick pushes on fsm_tx (a block
// was appended for a client's request) becomes a waiter (partition, block id, token = request id) registered by the next
// step that begins, and a sink receives the done rows when that step's outputs are consumed.  A few partitions follow and
// learn their leader from a Heartbeat halfway: a row of the general path, so that tick's chain comes back redone.
// Afterwards: every token arrived exactly once, JG_DONE_APPLIED, with block_id <= commit_now, in registration order per
// partition - and the table is empty.  Built and run by tests/test_cpp_awaited_loop.py (-m gpu).
#include <cstdio>
#include <cstring>
#include <map>
#include <set>

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
  const uint32_t G = 3000 + 37, T = 24;
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
  raft.open_waiters((size_t)G * 8);
  // fsm_tx: every Notify row is a waiter of the next step that begins, in the order the rows arrive
  std::vector<jg_await_row> fresh;
  std::map<uint64_t, std::pair<uint32_t, uint64_t>> issued;  // token -> (partition, block id)
  std::vector<std::vector<uint64_t>> order(G);                // per partition: its tokens in registration order
  uint64_t general = 0, msg_rows = 0;
  raft.fsm_rows_tx = [&](const jg_fsm_row* rows, size_t n) {
    for (size_t i = 0; i < n; i++) {
      if (rows[i].kind != JG_FSM_NOTIFY) continue;
      jg_await_row w{};
      w.group = rows[i].group, w.block_id = rows[i].a, w.token = rows[i].b;
      CHECK(!issued.count(w.token));
      issued[w.token] = {w.group, w.block_id};
      order[w.group].push_back(w.token);
      fresh.push_back(w);
    }
  };
  raft.msg_rows_tx = [&](const jg_msg_row*, size_t n) { msg_rows += n; };
  raft.columns_tx = [&](const jg_node_outbox& o) { general += o.rows_general; };
  std::set<uint64_t> answered;
  std::vector<size_t> next(G, 0);  // per partition: how many of its tokens have arrived
  uint64_t watches = 0, redone_watches = 0, registered = 0;
  loop.set_completions(
      [&](uint64_t) {
        std::vector<jg_await_row> rows;
        rows.swap(fresh);
        registered += rows.size();
        return rows;
      },
      [&](const std::vector<jg_done_row>& rows, bool redone) {
        watches++, redone_watches += redone;
        CHECK(rows.size() <= 1500);
        for (const jg_done_row& r : rows) {
          CHECK(r.state == JG_DONE_APPLIED);
          CHECK(r.group < G && issued.count(r.token));
          if (r.group >= G || !issued.count(r.token)) continue;
          CHECK(issued[r.token].first == r.group && issued[r.token].second == r.block_id);
          CHECK(r.block_id <= r.commit_now);
          CHECK(answered.insert(r.token).second);  // exactly once
          // registration order per partition
          CHECK(next[r.group] < order[r.group].size() && order[r.group][next[r.group]] == r.token);
          next[r.group]++;
        }
      },
      1500);  // (less than a busy tick completes: what is left is pending at the next tick)
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
    loop.run_until((uint64_t)t * BatchedEventLoop::TICK_MS);
  }
  // the last appends are acknowledged, then quiet ticks until everything registered has been delivered
  for (uint32_t t = T; t < T + 40 && (t < T + 4 || answered.size() < issued.size() || !fresh.empty()); t++) {
    RowQueue in;
    for (uint32_t g = 0; g < G && t == T; g++)
      if (!follows(g) && appended[g]) in.push(g, JG_CMD_APPEND_RESPONSE, ids[1], 1, appended[g], 0, 1);
    loop.tcp_rx_rows(in.view());
    loop.run_until((uint64_t)t * BatchedEventLoop::TICK_MS);
  }
  loop.flush();
  CHECK(watches >= T + 4);
  CHECK(redone_watches >= 1 && redone_watches < watches);
  CHECK(general > 0 && msg_rows > 0);
  CHECK(issued.size() > G && registered == issued.size() && fresh.empty());
  CHECK(answered.size() == issued.size());  // every token
  for (uint32_t g = 0; g < G; g++) CHECK(next[g] == order[g].size());
  // the table is empty: nothing is outstanding, the synchronous calls work again
  size_t total = 12345;
  jg_await_stats s{};
  const std::vector<jg_done_row> rest = raft.watch_completions(0, SIZE_MAX, true, &total, &s);
  CHECK(total == 0 && rest.empty() && s.left == 0 && s.waiting == 0);
  raft.open_waiters(0);
  if (g_failed) {
    std::fprintf(stderr, "%d checks failed (watches %llu, redone %llu, issued %zu, answered %zu)\n", g_failed, (unsigned long long)watches,
                 (unsigned long long)redone_watches, issued.size(), answered.size());
    return 1;
  }
  std::printf("awaited loop ok: %llu watches (%llu redone), %zu tokens\n", (unsigned long long)watches, (unsigned long long)redone_watches,
              issued.size());
  return 0;
}
