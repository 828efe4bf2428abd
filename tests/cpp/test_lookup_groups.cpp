// Point queries through the C++ host mirror (BatchedRaft::lookup: jg_engine_lookup_groups, ABI v16).  One broker (node id 2
// of the examples/multi-node ids 1, 2, 3) hosts 48 partitions: it wins the election of every third one and its clients
// append while one follower acknowledges, every fourth one learns its leader from a Heartbeat, a few campaign and stay
// candidates, a few are closed.  A list with repeats and the range form are then compared, row by row and field by field,
// with jg_read_state at the listed indices - what RaftHandle's getters read, one round trip each.  Built and run by
// tests/test_cpp_lookup_groups.py (-m gpu).
#include <cstdio>

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

static const uint32_t kG = 48, kR = 3;

template <class T>
static T read(BatchedRaft& b, int field, uint32_t g, uint32_t replica = 0) {
  T v{};
  if (jg_read_state(b.raw(), field, replica, &v, g, 1) != JG_OK) g_failed++;
  return v;
}

// row `r` (and its progress heads `m`, or nullptr) against jg_read_state of slot g
static void check_row(BatchedRaft& b, const jg_group_state& r, const uint64_t* m, uint32_t g) {
  CHECK(r.group == g);
  CHECK(r.term == read<uint64_t>(b, JG_FIELD_TERM, g) && r.head == read<uint64_t>(b, JG_FIELD_HEAD, g));
  CHECK(r.commit == read<uint64_t>(b, JG_FIELD_COMMIT, g) && r.id_gen == read<uint64_t>(b, JG_FIELD_ID_GEN, g));
  CHECK(r.election_time == read<uint64_t>(b, JG_FIELD_ELECTION_TIME, g));
  CHECK(r.heartbeat_time == read<uint64_t>(b, JG_FIELD_HEARTBEAT_TIME, g));
  CHECK(r.voted_for == read<uint32_t>(b, JG_FIELD_VOTED_FOR, g) && r.leader_id == read<uint32_t>(b, JG_FIELD_LEADER_ID, g));
  CHECK(r.election_timeout == read<uint32_t>(b, JG_FIELD_ELECTION_TIMEOUT, g));
  CHECK(r.queued_reqs == read<uint32_t>(b, JG_FIELD_QUEUED_REQS, g));
  CHECK(r.role == read<uint8_t>(b, JG_FIELD_ROLE, g) && r.fault == read<uint8_t>(b, JG_FIELD_FAULT, g));
  CHECK(r.self_slot == read<uint8_t>(b, JG_FIELD_SELF_SLOT, g) && r.repl_state == read<uint8_t>(b, JG_FIELD_REPL_STATE, g));
  CHECK(r.vote_seen == read<uint8_t>(b, JG_FIELD_VOTE_SEEN, g) && r.vote_granted == read<uint8_t>(b, JG_FIELD_VOTE_GRANTED, g));
  CHECK(r.has == (read<uint8_t>(b, JG_FIELD_HAS_VOTED, g) | read<uint8_t>(b, JG_FIELD_HAS_LEADER, g) << 1));
  // the leadership view, as jg_engine_watch_leaders defines it over the same columns
  const bool vacant = r.fault == JG_FAULT_VACANT, leads = r.role == JG_ROLE_LEADER, knows = (r.has & 2) != 0;
  const uint32_t want_state = vacant ? (uint32_t)JG_LEAD_VACANT
                                     : (leads ? JG_LEAD_KNOWN | JG_LEAD_SELF : knows ? (uint32_t)JG_LEAD_KNOWN : 0u) | (r.fault ? (uint32_t)JG_LEAD_FAULTED : 0u);
  CHECK(r.state == want_state);
  CHECK(r.known_leader == (vacant ? 0u : leads ? 2u : knows ? r.leader_id : 0u));
  if (m)
    for (uint32_t k = 0; k < kR; k++) CHECK(m[k] == read<uint64_t>(b, JG_FIELD_MATCH, g, k));
}

int main() {
  try {
    BatchedRaft b(kG, {1, 2, 3}, 0, 7, JG_CFG_SEPARATE_COMMIT_KEY);
    const std::vector<uint8_t> slots(kG, 1);  // node id 2 is member slot 1
    CHECK(jg_set_self_slots(b.raw(), slots.data()) == JG_OK);
    uint64_t now = 0, request = 0;
    uint32_t leaders = 0, informed = 0, candidates = 0;
    for (uint32_t g = 0; g < kG; g++) {
      if (g % 3 == 0) {  // elected: its own vote and node 3's
        b.apply(g, Command::Timeout(), now);
        b.apply(g, Command::VoteResponse(1, 3, true), now);
        CHECK(b.handle(g).is_leader());
        for (uint32_t k = 0; k <= g % 5; k++) b.apply(g, Command::ClientRequest(++request, {1, 2, 3}), now);
        b.apply(g, Command::AppendResponse(3, 1, b.handle(g).head() - (g % 2), true), now);  // node 1 never answers
        leaders++;
      } else if (g % 4 == 1) {  // a follower that hears from node 3 at term 4
        b.apply(g, Command::Heartbeat(4, 0, 3), now);
        informed++;
      } else if (g % 8 == 2) {  // a candidate without a quorum
        b.apply(g, Command::Timeout(), now);
        candidates++;
      }
    }
    b.close_groups({44, 46, 47});
    now += 150;
    b.apply(0, Command::Tick(), now);
    // a list in the request's own order, with repeats
    std::vector<uint32_t> list;
    for (uint32_t k = 0; k < 100; k++) list.push_back((k * 29 + 5) % kG);
    list.push_back(list[3]), list.push_back(list[3]), list.push_back(47), list.push_back(0);
    const BatchedRaft::GroupStates got = b.lookup(list.data(), list.size(), true);
    CHECK(got.rows.size() == list.size() && got.match.size() == list.size() * kR);
    uint32_t n_lead = 0, n_known = 0, n_cand = 0, n_vacant = 0, n_behind = 0;
    for (size_t i = 0; i < got.rows.size() && i < list.size(); i++) {
      const jg_group_state& r = got.rows[i];
      check_row(b, r, got.match.data() + i * kR, list[i]);
      n_lead += (r.state & JG_LEAD_SELF) != 0, n_known += r.state == JG_LEAD_KNOWN, n_cand += r.role == JG_ROLE_CANDIDATE;
      n_vacant += r.state == JG_LEAD_VACANT;
      if (r.state & JG_LEAD_SELF) n_behind += got.match[i * kR + 0] < r.head;  // node 1's progress
    }
    CHECK(n_lead >= leaders && n_known >= informed && n_cand >= candidates && n_vacant >= 3 && n_behind >= leaders);
    // without progress; the range form; nothing listed
    const BatchedRaft::GroupStates plain = b.lookup(list.data(), list.size());
    CHECK(plain.match.empty() && plain.rows.size() == got.rows.size());
    CHECK(std::memcmp(plain.rows.data(), got.rows.data(), got.rows.size() * sizeof(jg_group_state)) == 0);
    const uint32_t g0 = 5, n = 40;
    const BatchedRaft::GroupStates range = b.lookup(g0, n, true);
    CHECK(range.rows.size() == n);
    for (uint32_t i = 0; i < n && i < range.rows.size(); i++) check_row(b, range.rows[i], range.match.data() + i * kR, g0 + i);
    CHECK(b.lookup(list.data(), 0, true).rows.empty());
    // an index out of range is refused
    list.back() = kG;
    bool refused = false;
    try {
      b.lookup(list.data(), list.size());
    } catch (const EngineError&) {
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
  std::puts("lookup groups ok");
  return 0;
}
