// jg_api_feeds.h - the separate watch and census calls: jg_engine_watch_leaders, jg_engine_census (jg_watch.h),
// jg_engine_watch_replicas, jg_engine_replication_census (jg_isr.h), jg_engine_watch_replicas_timed (jg_isr_clock.h) and
// jg_engine_watch_commits (jg_commits.h).  Each is its own argument checks, the refusal while kept node steps are
// outstanding, and poll_handle (jg_api_poll.h) with ONE part wanted: the host path, the kernels and the launch order are
// the poll's, so what jg_engine_poll promises of a poll with one part - every output byte, every total, the backlog as the
// separate call leaves them - holds by construction.  Part of josefine_gpu.hip's one translation unit.
#pragma once

namespace {

// feed x alone, as `base` asks it (its peek and rules), over the handle's slots [g0, g0 + n)
int one_feed(jg_engine* e, PollShard& base, int x, uint32_t g0, uint32_t n, void* rows, size_t cap, size_t* total, uint64_t* backlog) {
  base.want = POLL_BIT[x];
  void* out[3] = {nullptr, nullptr, nullptr};
  size_t caps[3] = {0, 0, 0};
  size_t* tot[3] = {nullptr, nullptr, nullptr};
  out[x] = rows, caps[x] = cap, tot[x] = total;
  return poll_handle(e, base, g0, n, out, caps, tot, backlog, nullptr, nullptr);
}

// one census alone: `want` is its bit and w its words (only the wanted census is written)
int one_census(jg_engine* e, uint32_t want, uint64_t lag_limit, uint32_t g0, uint32_t n, uint64_t* w) {
  PollShard base;
  base.want = want, base.lag_limit = lag_limit;
  void* const out[3] = {nullptr, nullptr, nullptr};
  const size_t caps[3] = {0, 0, 0};
  size_t* const tot[3] = {nullptr, nullptr, nullptr};
  return poll_handle(e, base, g0, n, out, caps, tot, nullptr, w, w);
}

}  // namespace

extern "C" {

int jg_engine_watch_leaders(jg_engine* e, uint32_t flags, uint32_t g0, uint32_t n, jg_leader_row* out, size_t cap, size_t* total) {
  if (!e || !total || (cap && !out)) return fail(JG_EINVAL, "null argument");
  if (flags & ~(uint32_t)JG_WATCH_PEEK) return fail(JG_EINVAL, "jg_engine_watch_leaders: unknown flag");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_watch_leaders: slot range out of bounds");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  PollShard base;
  base.peek[POLL_L] = (flags & JG_WATCH_PEEK) != 0;
  return one_feed(e, base, POLL_L, g0, n, out, cap, total, nullptr);
}

int jg_engine_census(jg_engine* e, uint32_t g0, uint32_t n, jg_census* out) {
  if (!e || !out) return fail(JG_EINVAL, "null argument");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_census: slot range out of bounds");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  return one_census(e, JG_POLL_CENSUS, 0, g0, n, (uint64_t*)out);  // (jg_census is the census words in order: jg_watch.h)
}

int jg_engine_watch_replicas(jg_engine* e, uint32_t flags, const jg_isr_policy* p, uint32_t g0, uint32_t n, jg_isr_row* out, size_t cap,
                             size_t* total) {
  if (!e || !p || !total || (cap && !out)) return fail(JG_EINVAL, "null argument");
  if (flags & ~(uint32_t)JG_WATCH_PEEK) return fail(JG_EINVAL, "jg_engine_watch_replicas: unknown flag");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_watch_replicas: slot range out of bounds");
  if (p->join_lag > p->leave_lag) return fail(JG_EINVAL, "jg_engine_watch_replicas: join_lag above leave_lag");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  PollShard base;
  base.peek[POLL_I] = (flags & JG_WATCH_PEEK) != 0;
  base.pol = *p;
  return one_feed(e, base, POLL_I, g0, n, out, cap, total, nullptr);
}

int jg_engine_replication_census(jg_engine* e, uint64_t lag_limit, uint32_t g0, uint32_t n, jg_repl_census* out) {
  if (!e || !out) return fail(JG_EINVAL, "null argument");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_replication_census: slot range out of bounds");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  return one_census(e, JG_POLL_REPL_CENSUS, lag_limit, g0, n, (uint64_t*)out);  // (jg_repl_census is its words in order: jg_isr.h)
}

// (the peek of a timed watch says two things - the shadow AND the clocks are left alone: PollShard, jg_api_poll.h)
int jg_engine_watch_replicas_timed(jg_engine* e, uint32_t flags, const jg_isr_clock* c, uint32_t g0, uint32_t n, jg_isr_row* out, size_t cap,
                                   size_t* total) {
  if (!e || !c || !total || (cap && !out)) return fail(JG_EINVAL, "null argument");
  if (flags & ~(uint32_t)JG_WATCH_PEEK) return fail(JG_EINVAL, "jg_engine_watch_replicas_timed: unknown flag");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_watch_replicas_timed: slot range out of bounds");
  if (c->now_ms == UINT64_MAX) return fail(JG_EINVAL, "jg_engine_watch_replicas_timed: now_ms is UINT64_MAX");
  if (c->join_lag > c->caught_lag) return fail(JG_EINVAL, "jg_engine_watch_replicas_timed: join_lag above caught_lag");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  PollShard base;
  base.peek[POLL_I] = (flags & JG_WATCH_PEEK) != 0;
  base.timed = true, base.clk = *c;
  return one_feed(e, base, POLL_I, g0, n, out, cap, total, nullptr);
}

int jg_engine_watch_commits(jg_engine* e, uint32_t flags, uint32_t g0, uint32_t n, jg_commit_row* out, size_t cap, size_t* total,
                            jg_commit_backlog* backlog) {
  if (!e || !total || (cap && !out)) return fail(JG_EINVAL, "null argument");
  if (flags & ~(uint32_t)(JG_WATCH_PEEK | JG_WATCH_COMMITS_ONLY)) return fail(JG_EINVAL, "jg_engine_watch_commits: unknown flag");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_watch_commits: slot range out of bounds");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  PollShard base;
  base.peek[POLL_C] = (flags & JG_WATCH_PEEK) != 0, base.commits_only = (flags & JG_WATCH_COMMITS_ONLY) != 0;
  // (jg_commit_backlog is the backlog words in order: jg_commits.h)
  return one_feed(e, base, POLL_C, g0, n, out, cap, total, (uint64_t*)backlog);
}

}  // extern "C"
