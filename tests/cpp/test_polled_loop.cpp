// The feeds of a loop with two ticks in flight, through the C++ host mirror (BatchedEventLoop::set_poll over
// BatchedRaft::step_node_polled / node_poll: jg_step_node_polled / jg_node_poll_view, ABI v21).  ONE pipelined event loop with
// in_flight = 2 over a few thousand partitions this node leads; every tick's step carries a poll of the three feeds, small
// caps included, and a sink receives its answer when that tick's outputs are consumed.  Partitions are appended to and
// acknowledged at different rates; a few partitions follow and learn their leader from a Heartbeat halfway (a row of the
// general path in a loop that runs the leader half: that tick's poll comes back redone).  Afterwards: the concatenation of the sink's commit rows reproduces every partition's final
// (commit, head) from genesis, link by link, and the sink's leader rows end at the view the engine holds - watch_leaders
// peeks nothing more.  Built and run by tests/test_cpp_polled_loop.py (-m gpu).
#include <cstdio>
#include <cstring>
#include <map>

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
  uint64_t fsm_rows = 0, msg_rows = 0, general = 0;
  raft.fsm_rows_tx = [&](const jg_fsm_row*, size_t n) { fsm_rows += n; };
  raft.msg_rows_tx = [&](const jg_msg_row*, size_t n) { msg_rows += n; };
  raft.columns_tx = [&](const jg_node_outbox& o) { general += o.rows_general; };
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
  // the sink: per partition the chain of its commit rows, the last leader row, and how the polls came back
  std::vector<uint64_t> commit(G, 0), head(G, 0);
  std::map<uint32_t, jg_leader_row> leads;
  uint64_t polls = 0, redone_polls = 0, commit_rows = 0, leader_rows = 0, replica_rows = 0;
  BatchedRaft::PollRequest q;
  q.want = JG_POLL_LEADERS | JG_POLL_REPLICAS | JG_POLL_COMMITS | JG_POLL_CENSUS;
  q.policy = jg_isr_policy{2, 0};
  q.commits_limit = 1700;  // (less than a tick changes: what is left is pending at the next tick)
  q.leaders_limit = 900;
  loop.set_poll(q, [&](const BatchedRaft::PollResult& r, bool redone) {
    polls++, redone_polls += redone;
    CHECK(r.commits.size() == std::min<size_t>(r.commits_total, 1700));
    CHECK(r.census.hosted == G);
    for (const jg_commit_row& c : r.commits) {
      CHECK(c.group < G);
      if (c.group >= G) continue;
      CHECK(c.commit_from == commit[c.group] && c.head_from == head[c.group]);  // link by link from genesis
      commit[c.group] = c.commit, head[c.group] = c.head;
    }
    for (const jg_leader_row& l : r.leaders) leads[l.group] = l;
    commit_rows += r.commits.size(), leader_rows += r.leaders.size(), replica_rows += r.replicas.size();
  });
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
      if ((g + 2 * t) % 5) in.push(g, JG_CMD_CLIENT_REQUEST, 0, 0, (uint64_t)t * G + g), appended[g]++;
    }
    loop.tcp_rx_rows(in.view());
    loop.run_until((uint64_t)t * BatchedEventLoop::TICK_MS);
  }
  // a few quiet ticks: what the small caps left pending is delivered
  for (uint32_t t = T; t < T + 6; t++) loop.run_until((uint64_t)t * BatchedEventLoop::TICK_MS);
  loop.flush();
  CHECK(polls == T + 6);
  CHECK(redone_polls >= 1 && redone_polls < polls);
  CHECK(general > 0 && fsm_rows > 0);
  CHECK(commit_rows > G && leader_rows >= G && replica_rows > 0);
  // the chains end at the engine's state
  std::vector<uint64_t> h(G), c(G), term(G);
  std::vector<uint8_t> role(G);
  CHECK(jg_read_state(raft.raw(), JG_FIELD_HEAD, 0, h.data(), 0, G) == JG_OK);
  CHECK(jg_read_state(raft.raw(), JG_FIELD_COMMIT, 0, c.data(), 0, G) == JG_OK);
  CHECK(jg_read_state(raft.raw(), JG_FIELD_TERM, 0, term.data(), 0, G) == JG_OK);
  CHECK(jg_read_state(raft.raw(), JG_FIELD_ROLE, 0, role.data(), 0, G) == JG_OK);
  uint64_t moved = 0;
  for (uint32_t g = 0; g < G; g++) {
    CHECK(commit[g] == c[g] && head[g] == h[g]);
    moved += c[g] > 0;
  }
  CHECK(moved > G / 2);
  // ... and the leader rows at the view the engine holds: nothing is left to report, and the last row of a partition is it
  size_t total = 12345;
  const std::vector<jg_leader_row> rest = raft.watch_leaders(0, G, SIZE_MAX, true, &total);
  CHECK(total == 0 && rest.empty());
  CHECK(leads.size() == G);
  uint32_t followers = 0;
  for (const auto& kv : leads) {
    const jg_leader_row& l = kv.second;
    CHECK(l.role == role[l.group] && l.term == term[l.group]);
    if (follows(l.group)) {
      CHECK(l.role == JG_ROLE_FOLLOWER && (l.state & JG_LEAD_KNOWN) && l.leader_id == ids[2]);
      followers++;
    } else {
      CHECK(l.role == JG_ROLE_LEADER && (l.state & JG_LEAD_SELF));
    }
  }
  CHECK(followers > 0);
  // the commit feed too: nothing pending
  size_t pending = 12345;
  raft.watch_commits(0, G, SIZE_MAX, true, false, &pending, nullptr);
  CHECK(pending == 0);
  if (g_failed) {
    std::fprintf(stderr, "%d checks failed (polls %llu, redone %llu, commit rows %llu)\n", g_failed, (unsigned long long)polls,
                 (unsigned long long)redone_polls, (unsigned long long)commit_rows);
    return 1;
  }
  std::printf("polled loop ok: %llu polls (%llu redone), %llu commit rows, %llu leader rows, %llu replica rows\n", (unsigned long long)polls,
              (unsigned long long)redone_polls, (unsigned long long)commit_rows, (unsigned long long)leader_rows, (unsigned long long)replica_rows);
  return 0;
}
