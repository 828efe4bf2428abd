// One poll per tick through the C++ host mirror (BatchedRaft::poll: jg_engine_poll, ABI v18) against the three C++ watch
// calls and the two censuses on a TWIN.  Two clusters of three brokers each (ids 1, 2, 3; broker g % 3 leads partition g)
// run the same rounds on the device; after every eight rounds each broker of the first cluster is asked with watch_leaders,
// watch_replicas, watch_commits, census and replication_census, its twin in the second cluster with ONE poll - halfway the
// twins swap.  Everything returned is equal byte for byte, caps and peeks included.  Built and run by
// tests/test_cpp_poll.py (-m gpu).
#include <cstdio>
#include <cstring>
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

template <class Row>
static bool same_rows(const std::vector<Row>& a, const std::vector<Row>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(Row)) == 0);
}

// the separate calls of one request, as a PollResult
static BatchedRaft::PollResult separate(BatchedRaft& e, const BatchedRaft::PollRequest& q) {
  BatchedRaft::PollResult r;
  r.leaders = e.watch_leaders(q.g0, q.n, q.leaders_limit, q.leaders_peek, &r.leaders_total);
  r.replicas = e.watch_replicas(q.policy, q.g0, q.n, q.replicas_limit, q.replicas_peek, &r.replicas_total);
  r.commits = e.watch_commits(q.g0, q.n, q.commits_limit, q.commits_peek, q.commits_only, &r.commits_total, &r.backlog);
  r.census = e.census(q.g0, q.n);
  r.repl_census = e.replication_census(q.census_lag_limit, q.g0, q.n);
  return r;
}

static void check_equal(const BatchedRaft::PollResult& x, const BatchedRaft::PollResult& y) {
  CHECK(same_rows(x.leaders, y.leaders) && x.leaders_total == y.leaders_total);
  CHECK(same_rows(x.replicas, y.replicas) && x.replicas_total == y.replicas_total);
  CHECK(same_rows(x.commits, y.commits) && x.commits_total == y.commits_total);
  CHECK(std::memcmp(&x.backlog, &y.backlog, sizeof x.backlog) == 0);
  CHECK(std::memcmp(&x.census, &y.census, sizeof x.census) == 0);
  CHECK(std::memcmp(&x.repl_census, &y.repl_census, sizeof x.repl_census) == 0);
}

struct Cluster {
  std::vector<std::unique_ptr<BatchedRaft>> nodes;
  std::unique_ptr<LibraryCluster> lib;
  Cluster() {
    std::vector<jg_engine*> raw;
    for (uint32_t r = 0; r < 3; r++) {
      nodes.emplace_back(new BatchedRaft(kG, {1, 2, 3}, 0, 7 + r, JG_CFG_SEPARATE_COMMIT_KEY));
      const std::vector<uint8_t> slots(kG, (uint8_t)r);
      CHECK(jg_set_self_slots(nodes[r]->raw(), slots.data()) == JG_OK);
      raw.push_back(nodes[r]->raw());
    }
    for (uint32_t r = 0; r < 3; r++) {  // broker g % 3 wins partition g: Timeout, then a granted vote from the next broker
      for (uint32_t g = r; g < kG; g += 3) nodes[r]->submit(g, Command::Timeout());
      nodes[r]->step(0);
      for (uint32_t g = r; g < kG; g += 3) nodes[r]->submit(g, Command::VoteResponse(1, (r + 1) % 3 + 1, true));
      nodes[r]->step(0);
      CHECK(nodes[r]->handle(r).is_leader());
    }
    lib.reset(new LibraryCluster(raw, JG_CLUSTER_ANY_LEADER));
    lib->set_appends(1);
  }
};

int main() {
  try {
    Cluster a, b;
    size_t rows_seen = 0;
    for (uint32_t p = 0; p < 4; p++) {
      a.lib->rounds(100 + 800ull * p, 100, 8);
      b.lib->rounds(100 + 800ull * p, 100, 8);
      for (uint32_t r = 0; r < 3; r++) {
        BatchedRaft &sep = p < 2 ? *a.nodes[r] : *b.nodes[r], &pol = p < 2 ? *b.nodes[r] : *a.nodes[r];  // halfway the twins swap
        BatchedRaft::PollRequest q;
        q.want = JG_POLL_LEADERS | JG_POLL_REPLICAS | JG_POLL_COMMITS | JG_POLL_CENSUS | JG_POLL_REPL_CENSUS;
        q.policy = jg_isr_policy{2, 0};
        q.census_lag_limit = 1;
        // a peek with caps that differ between the feeds, over a range off the borders
        q.g0 = 3, q.n = kG - 7;
        q.leaders_peek = q.replicas_peek = q.commits_peek = true;
        q.leaders_limit = 1, q.replicas_limit = 0, q.commits_limit = 5;
        q.commits_only = true;
        check_equal(separate(sep, q), pol.poll(q));
        // a small cap loses nothing: the commits in pieces of 20, the leaders and the replicas whole, the replicas peeked once
        q = BatchedRaft::PollRequest();
        q.want = JG_POLL_LEADERS | JG_POLL_REPLICAS | JG_POLL_COMMITS | JG_POLL_CENSUS | JG_POLL_REPL_CENSUS;
        q.policy = jg_isr_policy{2, 0};
        q.commits_limit = 20;
        for (int piece = 0; piece < 3; piece++) {
          q.replicas_peek = piece == 0;
          const BatchedRaft::PollResult x = separate(sep, q), y = pol.poll(q);
          check_equal(x, y);
          CHECK(y.commits_total == kG - 20 * piece && y.commits.size() == (piece < 2 ? 20u : 8u));
          CHECK(y.census.leaders == kG / 3 && y.repl_census.leaders == kG / 3);
          rows_seen += y.commits.size();
        }
        q.want = JG_POLL_LEADERS | JG_POLL_REPLICAS | JG_POLL_COMMITS;
        const BatchedRaft::PollResult quiet = pol.poll(q);
        CHECK(quiet.leaders_total == 0 && quiet.replicas_total == 0 && quiet.commits_total == 0);
        CHECK(sep.watch_leaders().empty() && sep.watch_replicas(jg_isr_policy{2, 0}).empty() && sep.watch_commits().empty());
      }
    }
    CHECK(rows_seen == 4u * 3u * kG);
    // a part not named is not touched
    BatchedRaft::PollRequest q;
    q.want = JG_POLL_CENSUS;
    const BatchedRaft::PollResult c = a.nodes[0]->poll(q);
    CHECK(c.census.hosted == kG && c.leaders.empty() && c.commits_total == 0);
    q.want = 0;
    bool refused = false;
    try {
      a.nodes[0]->poll(q);
    } catch (const std::exception&) {
      refused = true;
    }
    CHECK(refused);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  if (g_failed) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failed);
    return 1;
  }
  std::puts("poll ok");
  return 0;
}
