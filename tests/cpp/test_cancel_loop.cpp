// Withdrawing waiters from a loop with two ticks in flight, through the C++ host mirror (BatchedEventLoop::cancel_tokens over
// BatchedRaft::step_node_awaited: jg_node_await_request.cancel_keys, ABI v24).  The scenario of tests/cpp/test_awaited_loop.cpp
// - ONE pipelined event loop with in_flight = 2 over a few thousand partitions this node leads, every Notify row a waiter of
// the next step that begins - with tokens that carry a CONNECTION id in their high half (a partition's clients share one).
// A third of the connections close mid-run: cancel_tokens(their ids << 32, the high mask) travels with the next step.  From
// that step's watch on, every token of a closed connection arrives JG_DONE_CANCELLED and none of them applied; before it,
// and for every other connection, applied.  Every token arrives exactly once, in registration order per partition, and the
// table ends empty.  Built and run by tests/test_cpp_cancel_loop.py (-m gpu).
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
  const uint32_t CONNS = 12;
  const uint64_t HIGH = 0xFFFFFFFF00000000ull;
  auto conn_of = [&](uint32_t g) { return (uint64_t)(g % CONNS + 1); };
  auto closes = [](uint64_t conn) { return conn % 3 == 0; };  // a third of the connections hang up at tick T / 2
  const uint32_t QUIET = T / 2 - 4;  // their last requests: every Notify row of theirs is registered before the close
  bool closed = false;               // cancel_tokens has been called
  uint64_t steps_begun = 0, cancel_step = UINT64_MAX;  // awaited steps begun; the one the cancel travels with
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
      CHECK(w.token >> 32 == conn_of(w.group));
      CHECK(!(closed && closes(w.token >> 32)));  // a condition of the test: nothing of a closed connection registers after the close
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
  uint64_t watches = 0, redone_watches = 0, registered = 0, cancelled = 0, applied_closed = 0;
  loop.set_completions(
      [&](uint64_t) {
        std::vector<jg_await_row> rows;
        rows.swap(fresh);
        registered += rows.size();
        if (closed && cancel_step == UINT64_MAX) cancel_step = steps_begun;  // (the key set travels with this step)
        steps_begun++;
        return rows;
      },
      [&](const std::vector<jg_done_row>& rows, bool redone) {
        const bool behind = watches >= cancel_step;  // the watch of the step the cancel travelled with, or a later one
        watches++, redone_watches += redone;
        CHECK(rows.size() <= 1500);
        for (const jg_done_row& r : rows) {
          CHECK(r.group < G && issued.count(r.token));
          if (r.group >= G || !issued.count(r.token)) continue;
          if (behind && closes(r.token >> 32)) {
            CHECK(r.state == JG_DONE_CANCELLED);  // and not applied, whatever its slot's commit says
            cancelled++;
          } else {
            CHECK(r.state == JG_DONE_APPLIED);
            CHECK(r.block_id <= r.commit_now);
            applied_closed += closes(r.token >> 32);
          }
          CHECK(issued[r.token].first == r.group && issued[r.token].second == r.block_id);
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
      // the member acknowledges what it has - but not, from three ticks before their last requests to the end of the run, on
      // the partitions of the connections that close: their last blocks are outstanding at the close and commit behind it
      const bool held = closes(conn_of(g)) && t + 3 > QUIET;
      if (appended[g] && !held) in.push(g, JG_CMD_APPEND_RESPONSE, ids[1], 1, appended[g], 0, 1);
      if (closes(conn_of(g)) && t > QUIET) continue;  // the connection is about to hang up, or has
      if ((g + 2 * t) % 5) in.push(g, JG_CMD_CLIENT_REQUEST, 0, 0, conn_of(g) << 32 | ((uint64_t)t * G + g + 1)), appended[g]++;
    }
    if (t == T / 2) {  // the connections close: their ids as keys under the high mask, in two calls that the loop merges
      std::vector<uint64_t> a, b;
      for (uint64_t c = 1; c <= CONNS; c++)
        if (closes(c)) (c % 2 ? a : b).push_back(c << 32);
      loop.cancel_tokens(a, HIGH);
      loop.cancel_tokens(b, HIGH);
      closed = true;
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
  CHECK(cancel_step != UINT64_MAX && cancel_step > 2 && cancel_step < watches);
  CHECK(cancelled > G / 10 && applied_closed > 0);  // tokens of closed connections arrived both ways: applied before, cancelled behind
  for (uint32_t g = 0; g < G; g++) CHECK(next[g] == order[g].size());
  // the table is empty: nothing is outstanding, the synchronous calls work again
  size_t total = 12345;
  jg_await_stats s{};
  const std::vector<jg_done_row> rest = raft.watch_completions(0, SIZE_MAX, true, &total, &s);
  CHECK(total == 0 && rest.empty() && s.left == 0 && s.waiting == 0);
  raft.open_waiters(0);
  if (g_failed) {
    std::fprintf(stderr, "%d checks failed (watches %llu, redone %llu, issued %zu, answered %zu, cancelled %llu)\n", g_failed,
                 (unsigned long long)watches, (unsigned long long)redone_watches, issued.size(), answered.size(), (unsigned long long)cancelled);
    return 1;
  }
  std::printf("cancel loop ok: %llu watches (%llu redone), %zu tokens, %llu cancelled\n", (unsigned long long)watches,
              (unsigned long long)redone_watches, issued.size(), (unsigned long long)cancelled);
  return 0;
}
