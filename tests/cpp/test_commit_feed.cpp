// The commit feed through the C++ host mirror (BatchedRaft::watch_commits / as_fsm_rows: jg_engine_watch_commits, ABI v17).
// Three BatchedRafts - three brokers with the examples/multi-node ids 1, 2, 3 - host the same 48 partitions in one
// jg_dense_cluster; broker g % 3 leads partition g, clients append every round, and the rounds run on the device, eight at
// a time: they queue no FSM rows.  Each broker's view of what is committed - here a set of applied block keys per partition -
// is advanced ONLY from its feed: watch_commits, as_fsm_rows, and the ranges the rows stand for (a leader: keys (a, b]; a
// follower: keys [a, b)).  At the end every set holds exactly the keys up to that broker's commit column.  Built and run by
// tests/test_cpp_commit_feed.py (-m gpu).
#include <cstdio>
#include <memory>
#include <set>

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
      size_t total = 7;  // a fresh engine holds genesis only: the feed is empty
      CHECK(nodes[r]->watch_commits(0, UINT32_MAX, SIZE_MAX, false, false, &total).empty() && total == 0);
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
    std::vector<std::vector<std::set<uint64_t>>> applied(3, std::vector<std::set<uint64_t>>(kG));
    std::vector<std::vector<uint64_t>> head(3, std::vector<uint64_t>(kG, 0));
    size_t rows_seen = 0;
    for (uint32_t p = 0; p < 5; p++) {
      cl.rounds(100 + 800ull * p, 100, 8);
      for (uint32_t r = 0; r < 3; r++) {
        size_t total = 0;
        jg_commit_backlog backlog{};
        const std::vector<jg_commit_row> peek = nodes[r]->watch_commits(0, UINT32_MAX, 5, true, false, &total, &backlog);
        CHECK(total == kG && peek.size() == 5 && backlog.changed == total && backlog.rewound == 0);
        // a small cap loses nothing: the partitions in pieces of 20
        std::vector<jg_commit_row> rows;
        for (int piece = 0; piece < 3; piece++) {
          const std::vector<jg_commit_row> part = nodes[r]->watch_commits(0, UINT32_MAX, 20, false, false, &total);
          CHECK(total == kG - 20 * piece && part.size() == (piece < 2 ? 20u : 8u));
          rows.insert(rows.end(), part.begin(), part.end());
        }
        CHECK(rows.size() == kG && std::memcmp(&rows[0], &peek[0], 5 * sizeof(jg_commit_row)) == 0);
        CHECK(nodes[r]->watch_commits().empty());
        rows_seen += rows.size();
        uint64_t pending = 0;
        for (const jg_commit_row& row : rows) {
          const bool leads = row.group % 3 == r;
          CHECK(((row.state & JG_CMT_LEADS) != 0) == leads && !(row.state & (JG_CMT_REWOUND | JG_CMT_VACANT | JG_CMT_FAULTED)));
          CHECK(row.head_from == head[r][row.group] && row.head > row.head_from && row.term == 1 && row.self_slot == r);
          head[r][row.group] = row.head;
          pending += row.commit - row.commit_from;
        }
        CHECK(pending == backlog.pending_commits);
        for (const jg_fsm_row& f : BatchedRaft::as_fsm_rows(rows)) {
          std::set<uint64_t>& keys = applied[r][f.group];
          const uint64_t lo = f.kind == JG_FSM_APPLY_LEADER ? f.a + 1 : f.a, hi = f.kind == JG_FSM_APPLY_LEADER ? f.b + 1 : f.b;
          for (uint64_t k = lo; k < hi; k++) CHECK(keys.insert(k).second);  // (consecutive ranges concatenate exactly: no key twice)
        }
      }
    }
    CHECK(rows_seen == 5u * 3u * kG);
    // every broker's applied keys are exactly the keys up to its commit column: (0, commit] where it leads, [0, commit) where it follows
    for (uint32_t r = 0; r < 3; r++) {
      for (uint32_t g = 0; g < kG; g++) {
        RaftHandle h = nodes[r]->handle(g);
        const uint64_t commit = h.commit();
        const bool leads = g % 3 == r;
        CHECK(h.fault() == 0 && h.is_leader() == leads && commit >= 30 && h.head() == head[r][g]);
        const std::set<uint64_t>& keys = applied[r][g];
        CHECK(keys.size() == commit && *keys.begin() == (leads ? 1u : 0u) && *keys.rbegin() == (leads ? commit : commit - 1));
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("commit feed ok");
  return 0;
}
