// The completion feed through the C++ host mirror (BatchedRaft::open_waiters / await_blocks / watch_completions:
// jg_engine_await_open / _await_blocks / _watch_completions, ABI v22).  Three BatchedRafts - three brokers with the
// examples/multi-node ids 1, 2, 3 - host the same 48 partitions in one jg_dense_cluster; broker g % 3 leads partition g,
// clients append every round, and the rounds run on the device, eight at a time: they queue no FSM rows.  Each leader
// registers a waiter per appended id from its commit feed (ids (head_from, head], guarded by the row's term) and every
// request is answered exactly once through watch_completions, as applied, no later than the commit column covers its id.
// Built and run by tests/test_cpp_completion_feed.py (-m gpu).
#include <cstdio>
#include <map>
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

static const uint32_t kG = 48;  // partitions per broker

int main() {
  try {
    std::vector<std::unique_ptr<BatchedRaft>> nodes;
    std::vector<jg_engine*> raw;
    for (uint32_t r = 0; r < 3; r++) {
      nodes.emplace_back(new BatchedRaft(kG, {1, 2, 3}, 0, 7 + r, JG_CFG_SEPARATE_COMMIT_KEY));
      const std::vector<uint8_t> slots(kG, (uint8_t)r);
      CHECK(jg_set_self_slots(nodes[r]->raw(), slots.data()) == JG_OK);
      raw.push_back(nodes[r]->raw());
      size_t total = 7;  // no table yet: a watch answers nothing
      CHECK(nodes[r]->watch_completions(0, SIZE_MAX, false, &total).empty() && total == 0);
      nodes[r]->open_waiters(4096);
    }
    // broker g % 3 wins partition g the reference's way: Timeout, then a granted vote from the next broker
    for (uint32_t r = 0; r < 3; r++) {
      for (uint32_t g = r; g < kG; g += 3) nodes[r]->submit(g, Command::Timeout());
      nodes[r]->step(0);
      for (uint32_t g = r; g < kG; g += 3) nodes[r]->submit(g, Command::VoteResponse(1, (r + 1) % 3 + 1, true));
      nodes[r]->step(0);
      CHECK(nodes[r]->handle(r).is_leader());
    }
    LibraryCluster cl(raw, JG_CLUSTER_ANY_LEADER);
    cl.set_appends(1);
    // per broker: the requests in flight, token -> (partition, block id)
    std::vector<std::map<uint64_t, std::pair<uint32_t, uint64_t>>> parked(3);
    uint64_t next_token = 1, asked = 0, answered = 0;
    for (uint32_t p = 0; p < 6; p++) {
      if (p == 5) cl.set_appends(0);  // the last rounds only acknowledge: everything in flight commits
      cl.rounds(100 + 800ull * p, 100, 8);
      for (uint32_t r = 0; r < 3; r++) {
        std::vector<jg_await_row> waiters;
        for (const jg_commit_row& row : nodes[r]->watch_commits()) {
          if (!(row.state & JG_CMT_APPENDED) || !(row.state & JG_CMT_LEADS)) continue;
          CHECK(row.group % 3 == r);
          for (uint64_t id = row.head_from + 1; id <= row.head; id++) {
            jg_await_row w{};
            w.group = row.group, w.token = next_token, w.block_id = id, w.term = row.term;
            parked[r][next_token++] = {row.group, id};
            waiters.push_back(w);
          }
        }
        asked += waiters.size();
        nodes[r]->await_blocks(waiters);
        size_t total = 0;
        jg_await_stats st{};
        const std::vector<jg_done_row> peek = nodes[r]->watch_completions(0, 3, true, &total, &st);
        CHECK(st.done == total && st.waiting + st.done == parked[r].size() && st.left == parked[r].size() && st.lost == 0 && st.expired == 0);
        CHECK(peek.size() == std::min<size_t>(3, total));
        // a small cap loses nothing: the answers in pieces of 50, in registration order
        uint64_t last = 0;
        size_t got = 0;
        for (;;) {
          const std::vector<jg_done_row> part = nodes[r]->watch_completions(0, 50, false, &total);
          if (part.empty()) break;
          for (const jg_done_row& d : part) {
            if (got < peek.size()) CHECK(std::memcmp(&d, &peek[got], sizeof d) == 0);
            got++;
            auto it = parked[r].find(d.token);
            CHECK(it != parked[r].end());  // every request once
            if (it == parked[r].end()) continue;
            CHECK(d.state == JG_DONE_APPLIED && d.group == it->second.first && d.block_id == it->second.second);
            CHECK(d.block_id <= d.commit_now && d.term_now == 1 && d.self_slot == r && d.token > last);
            last = d.token;
            parked[r].erase(it);
            answered++;
          }
        }
        CHECK(got == st.done);
        // what is still parked is exactly what the commit column does not cover yet
        for (const auto& kv : parked[r]) CHECK(kv.second.second > nodes[r]->handle(kv.second.first).commit());
      }
    }
    CHECK(asked > 30u * kG && answered == asked);
    for (uint32_t r = 0; r < 3; r++) {
      CHECK(parked[r].empty());
      nodes[r]->open_waiters(0);  // the table is empty: it can be freed
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("completion feed ok");
  return 0;
}
