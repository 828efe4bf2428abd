// Partitions opened and closed in a loop with two ticks in flight, through the C++ host mirror (BatchedEventLoop::open_async /
// close_async over BatchedRaft::step_node_hosted / node_hosting: jg_step_node_hosted / jg_node_hosting_view, ABI v26).  ONE
// pipelined event loop with in_flight = 2 over a few thousand partitions this node leads, clients appending all the time:
// every tick closes a random list of hosted partitions and opens a random list of vacant ones - some of them closed by the
// very same tick's request - and a sink hears the verdict when the outputs of the tick that carried the request are
// consumed.  A few partitions follow and learn their leader from a Heartbeat halfway: a row of the general path, so that
// tick's hosting pass comes back redone.  Every sink is called exactly once, in request order; one request is refused (it
// closes a vacant slot) and the open beside it is applied all the same.  Partitions opened by tick t get a Timeout with tick
// t + 1's rows - handed to the loop before tick t's outputs are consumed - and a granted vote a tick later: they lead again,
// at term 1, from Chain::new's genesis.  Afterwards the engine's hosted set equals the host's own bookkeeping, and on a loop
// below two in flight the synchronous calls are made at the step boundary.  Built and run by
// tests/test_cpp_hosted_loop.py (-m gpu).
#include <algorithm>
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
  (void)R;
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
  uint64_t general = 0, notified = 0;
  raft.fsm_rows_tx = [&](const jg_fsm_row* rows, size_t n) {
    for (size_t i = 0; i < n; i++) notified += rows[i].kind == JG_FSM_NOTIFY;
  };
  raft.msg_rows_tx = [&](const jg_msg_row*, size_t) {};
  raft.columns_tx = [&](const jg_node_outbox& o) { general += o.rows_general; };

  // the host's own bookkeeping: a request changes it when it is made (the requests are made in an order that applies)
  std::vector<uint8_t> hosted(G, 1), touched(G, 0);
  std::mt19937 rng(11);
  size_t asked = 0, answered = 0, refused = 0, redone_answers = 0;
  auto sink_for = [&](bool applies) {
    const size_t seq = asked++;
    return [&, seq, applies](bool applied, bool redone) {
      CHECK(seq == answered);  // exactly once, in request order
      answered++;
      CHECK(applied == applies);
      refused += !applied, redone_answers += redone;
    };
  };
  auto take = [&](uint8_t state, size_t n, std::vector<uint32_t> extra = {}) {  // n random slots in `state` (and `extra`), ascending
    std::vector<uint32_t> pool;
    for (uint32_t g = 0; g < G; g++)
      if (hosted[g] == state && !follows(g)) pool.push_back(g);
    std::shuffle(pool.begin(), pool.end(), rng);
    pool.resize(std::min(n, pool.size()));
    pool.insert(pool.end(), extra.begin(), extra.end());
    std::sort(pool.begin(), pool.end());
    pool.erase(std::unique(pool.begin(), pool.end()), pool.end());
    return pool;
  };

  std::vector<uint64_t> appended(G, 0);
  std::vector<std::vector<uint32_t>> opened_at(T + 3);
  std::vector<uint32_t> reopened;  // opened by a tick and campaigning since
  std::vector<int> last_open(G, -1), voted_for_open(G, -1);  // the tick of a slot's latest open; the open its granted vote answered
  for (uint32_t t = 0; t < T; t++) {
    RowQueue in;
    for (uint32_t g = 0; g < G; g++) {
      if (follows(g)) {  // its leader's Heartbeat: the follower learns who leads (the general path: the follower half does not run)
        if (t == T / 2) in.push(g, JG_CMD_HEARTBEAT, ids[2], 1, 0, 0, 0);
        continue;
      }
      if (touched[g] || (g + t) % 3 == 0) continue;  // closed or reopened (below), or quiet this tick
      if (appended[g]) in.push(g, JG_CMD_APPEND_RESPONSE, ids[1], 1, appended[g], 0, 1);
      if ((g + 2 * t) % 5) in.push(g, JG_CMD_CLIENT_REQUEST, 0, 0, (uint64_t)t * G + g + 1), appended[g]++;
    }
    // what tick t - 1 opened campaigns with THIS tick's rows (its outputs have not been consumed yet), and wins a tick later
    if (t >= 1)
      for (uint32_t g : opened_at[t - 1]) in.push(g, JG_CMD_TIMEOUT);
    if (t >= 2)
      for (uint32_t g : opened_at[t - 2]) in.push(g, JG_CMD_VOTE_RESPONSE, ids[1], 1, 0, 0, 1), reopened.push_back(g), voted_for_open[g] = (int)t - 2;
    loop.tcp_rx_rows(in.view());
    const bool opening = t >= 1 && t < T - 3;
    if (t == 5) {  // a close that names a vacant slot is refused as a whole; the open beside it is applied
      std::vector<uint32_t> bad = take(1, 20), vac = take(0, 1);
      CHECK(!vac.empty());
      bad.push_back(vac[0]);
      std::sort(bad.begin(), bad.end());
      loop.close_async(bad, sink_for(false));
    } else {
      const std::vector<uint32_t> c = take(1, t % 4 == 3 ? 0 : 1 + rng() % 200);
      for (uint32_t g : c) hosted[g] = 0, touched[g] = 1;
      loop.close_async(c, sink_for(true));
      if (opening && t % 3 == 1 && !c.empty()) opened_at[t].assign(c.begin(), c.begin() + std::min<size_t>(c.size(), 3));  // closed and reopened by one step
    }
    if (opening) {
      const std::vector<uint32_t> o = take(0, 1 + rng() % 60, opened_at[t]);
      for (uint32_t g : o) hosted[g] = 1, last_open[g] = (int)t;
      opened_at[t] = o;
      if (t % 2) loop.open_async(o, std::vector<uint8_t>(o.size(), 0), sink_for(true));  // (the own slot named: the engine's uniform one)
      else loop.open_async(o, {}, sink_for(true));
    }
    loop.run_until((uint64_t)t * BatchedEventLoop::TICK_MS);
  }
  for (uint32_t t = T; t < T + 4; t++) loop.run_until((uint64_t)t * BatchedEventLoop::TICK_MS);
  loop.flush();
  CHECK(answered == asked && asked >= 2 * T - 6);
  CHECK(refused == 1);
  CHECK(redone_answers >= 1 && redone_answers < answered);
  CHECK(general > 0 && notified > G);
  auto same_sets = [&] {
    std::vector<uint32_t> want;
    for (uint32_t g = 0; g < G; g++)
      if (hosted[g]) want.push_back(g);
    CHECK(raft.hosted_groups() == want);
    CHECK(raft.vacant_groups().size() == G - want.size());
  };
  same_sets();
  // a reopened partition elects again: it leads at term 1, whatever term the slot had before
  {
    std::sort(reopened.begin(), reopened.end());
    reopened.erase(std::unique(reopened.begin(), reopened.end()), reopened.end());
    // (hosted at the end and the vote answered its latest open: it was neither closed nor opened again since it campaigned)
    std::vector<uint32_t> still;
    for (uint32_t g : reopened)
      if (hosted[g] && voted_for_open[g] == last_open[g]) still.push_back(g);
    CHECK(still.size() >= 20);
    const BatchedRaft::GroupStates s = raft.lookup(still.data(), still.size(), false);
    size_t leads = 0;
    for (const jg_group_state& r : s.rows) {
      CHECK(r.fault == 0);
      leads += r.role == JG_ROLE_LEADER && r.term == 1;
    }
    CHECK(leads == still.size());
  }
  // on a loop below two in flight no step is kept: the synchronous calls at the next step boundary, in the order asked
  {
    loop.in_flight = 1;
    const std::vector<uint32_t> c = take(1, 50);
    for (uint32_t g : c) hosted[g] = 0;
    loop.close_async(c, sink_for(true));
    loop.open_async(c, {}, sink_for(true));  // (what the call before closed)
    for (uint32_t g : c) hosted[g] = 1;
    loop.open_async(c, {}, sink_for(false));  // (hosted by now: refused)
    const size_t before = answered;
    loop.run_until((uint64_t)(T + 5) * BatchedEventLoop::TICK_MS);
    CHECK(answered == before + 3 && answered == asked);
    loop.flush();
    same_sets();
  }
  if (g_failed) {
    std::fprintf(stderr, "%d checks failed (asked %zu, answered %zu, redone %zu)\n", g_failed, asked, answered, redone_answers);
    return 1;
  }
  std::printf("hosted loop ok: %zu requests (%zu redone, %zu refused)\n", answered, redone_answers, refused);
  return 0;
}
