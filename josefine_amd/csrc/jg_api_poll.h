// jg_api_poll.h - jg_engine_poll: the three change feeds and the two censuses of one tick in one call (jg_poll.h).  A call
// that reads, under the rules of jg_api_manage.h and in the shape of jg_api_commits.h: every argument of every wanted part
// checked before anything is queued, refused while kept node steps are outstanding, JG_NODE_ASYNC steps settled ONCE, one
// block of scratch carved from the engine's staging for all parts, ONE count pass, one scan launch, the feeds' own write
// passes and the census kernels queued back to back, the small answers copied asynchronously, ONE synchronisation, then
// the rows of the feeds that have any.  A multi-device handle is served shard by shard.  Part of josefine_gpu.hip's one
// translation unit.
#pragma once

namespace {

enum { POLL_L = 0, POLL_I = 1, POLL_C = 2 };  // the feeds in the order a consumer reads them

// one single-device engine's part of a poll: shard-local slots [g0, g0 + n); per wanted feed x the first cap[x] changed
// rows (groups + add) into host out[x], their shadow advanced unless peek[x], total[x] the slots that differ; the parts not
// wanted are neither computed nor touched.  With `timed` the replicas part is under the time rule of `clk` (pol is not
// read), and peek[POLL_I] says two things: the shadow of the delivered rows is left alone, as for the other feeds, AND the
// clocks of the range are - without it they advance to clk.now_ms whatever cap[POLL_I] is, 0 included
struct PollShard {
  uint32_t want = 0;  // JG_POLL_*
  uint32_t g0 = 0, n = 0, add = 0;
  bool peek[3] = {false, false, false};
  bool commits_only = false;
  jg_isr_policy pol{};
  bool timed = false;
  jg_isr_clock clk{};
  uint64_t lag_limit = 0;
  void* out[3] = {nullptr, nullptr, nullptr};
  size_t cap[3] = {0, 0, 0}, total[3] = {0, 0, 0};
  uint64_t* backlog = nullptr;  // [JG_CMT_WORDS] of the range before the delivery, or null
  uint64_t census[JG_CENSUS_WORDS] = {};
  uint64_t repl[JG_RC_WORDS] = {};
};

const uint32_t POLL_BIT[3] = {JG_POLL_LEADERS, JG_POLL_REPLICAS, JG_POLL_COMMITS};
const size_t POLL_ROW[3] = {sizeof(jg_leader_row), sizeof(jg_isr_row), sizeof(jg_commit_row)};

int poll_shard(jg_engine* e, PollShard& q) {
  for (size_t& t : q.total) t = 0;
  if (q.backlog) std::memset(q.backlog, 0, JG_CMT_WORDS * 8);
  std::memset(q.census, 0, sizeof q.census);
  std::memset(q.repl, 0, sizeof q.repl);
  if (!q.n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = node_settle(e);
    if (rc) return rc;
  }
  const bool on[3] = {(q.want & JG_POLL_LEADERS) != 0, (q.want & JG_POLL_REPLICAS) != 0, (q.want & JG_POLL_COMMITS) != 0};
  const bool census = (q.want & JG_POLL_CENSUS) != 0, repl = (q.want & JG_POLL_REPL_CENSUS) != 0;
  const bool backlog = on[POLL_C] && q.backlog;
  // (zero-filled on the engine's stream; only the wanted feeds': an engine that never watches a feed does not pay for it)
  if (on[POLL_L] && !e->watch_shadow)
    if (const int rc = dev_alloc(e, &e->watch_shadow, e->cfg.n_groups)) return rc;
  if (on[POLL_I] && !e->isr_shadow)
    if (const int rc = dev_alloc(e, &e->isr_shadow, e->cfg.n_groups)) return rc;
  const bool timed = on[POLL_I] && q.timed;
  if (timed && !e->isr_stamp)  // (the clocks, as isr_clock_shard allocates them: no member was behind at the last sample)
    if (const int rc = dev_alloc(e, &e->isr_stamp, (size_t)e->cfg.n_replicas * e->cfg.n_groups)) return rc;
  if (timed && !e->isr_behind)
    if (const int rc = dev_alloc(e, &e->isr_behind, e->cfg.n_groups)) return rc;
  if (on[POLL_C] && !e->commit_shadow)
    if (const int rc = dev_alloc(e, &e->commit_shadow, e->cfg.n_groups)) return rc;
  JgPollArgs a{};
  a.tiles = (q.n + JG_POLL_TILE - 1) / JG_POLL_TILE;
  a.parts = std::min<uint32_t>(a.tiles, JG_CMT_PARTS);
  JgCensusArgs ca{};
  ca.g0 = q.g0, ca.n = q.n, ca.tiles = (q.n + JG_CENSUS_TILE - 1) / JG_CENSUS_TILE;
  JgReplCensusArgs ra{};
  ra.g0 = q.g0, ra.n = q.n, ra.lag_limit = q.lag_limit;
  ra.tiles = (q.n + JG_REPL_CENSUS_TILE - 1) / JG_REPL_CENSUS_TILE;
  ra.parts = std::min<uint32_t>(ra.tiles, JG_REPL_CENSUS_PARTS);
  size_t wcap[3], o_cnt[3], o_bsum[3], o_out[3];
  uint32_t feeds = 0;
  Carve c;
  const size_t o_total = c.sect(3 * 8), o_job = c.sect(3 * sizeof(JgScanJob)), o_sum = c.sect(JG_CMT_WORDS * 8),
               o_part = c.sect(backlog ? (size_t)a.parts * JG_CMT_WORDS * 8 : 0);
  for (int x = 0; x < 3; x++) {
    wcap[x] = on[x] ? std::min<size_t>(q.cap[x], q.n) : 0;
    o_cnt[x] = c.sect(on[x] ? (size_t)a.tiles * 4 : 0), o_bsum[x] = c.sect(on[x] ? (size_t)a.tiles * 8 : 0);
    o_out[x] = c.sect(wcap[x] * POLL_ROW[x]);
    feeds += on[x] ? 1u : 0u;
  }
  const size_t o_cen = c.sect(JG_CENSUS_WORDS * 8), o_cen_part = c.sect(census ? (size_t)ca.tiles * JG_CENSUS_WORDS * 8 : 0),
               o_rc = c.sect(JG_RC_WORDS * 8), o_rc_part = c.sect(repl ? (size_t)ra.parts * JG_RC_WORDS * 8 : 0);
  char* B = nullptr;
  if (const int rc = c.on_staging(e, B)) return rc;
  a.lw.g0 = a.ir.g0 = a.cm.g0 = q.g0, a.lw.n = a.ir.n = a.cm.n = q.n, a.lw.add = a.ir.add = a.cm.add = q.add;
  a.lw.peek = q.peek[POLL_L] ? 1u : 0u, a.ir.peek = q.peek[POLL_I] ? 1u : 0u, a.cm.peek = q.peek[POLL_C] ? 1u : 0u;
  a.lw.shadow = e->watch_shadow, a.ir.shadow = e->isr_shadow, a.cm.shadow = e->commit_shadow;
  a.lw.cnt = (uint32_t*)(B + o_cnt[POLL_L]), a.ir.cnt = (uint32_t*)(B + o_cnt[POLL_I]), a.cm.cnt = (uint32_t*)(B + o_cnt[POLL_C]);
  a.lw.bsum = (uint64_t*)(B + o_bsum[POLL_L]), a.ir.bsum = (uint64_t*)(B + o_bsum[POLL_I]), a.cm.bsum = (uint64_t*)(B + o_bsum[POLL_C]);
  a.lw.out = (jg_leader_row*)(B + o_out[POLL_L]), a.ir.out = (jg_isr_row*)(B + o_out[POLL_I]), a.cm.out = (uint4*)(B + o_out[POLL_C]);
  a.lw.cap = wcap[POLL_L], a.ir.cap = wcap[POLL_I], a.cm.cap = wcap[POLL_C];
  a.ir.leave_lag = q.pol.leave_lag, a.ir.join_lag = q.pol.join_lag;
  if (timed) {  // (the same feed: the shadow, the scratch and the rows are the lag rule's)
    a.ic.g0 = q.g0, a.ic.n = q.n, a.ic.add = q.add, a.ic.peek = a.ir.peek;
    a.ic.now1 = q.clk.now_ms + 1, a.ic.max_behind_ms = q.clk.max_behind_ms, a.ic.caught_lag = q.clk.caught_lag, a.ic.join_lag = q.clk.join_lag;
    a.ic.shadow = e->isr_shadow, a.ic.stamp = e->isr_stamp, a.ic.mask = e->isr_behind;
    a.ic.cnt = a.ir.cnt, a.ic.bsum = a.ir.bsum, a.ic.out = a.ir.out, a.ic.cap = a.ir.cap;
  }
  a.cm.commits_only = q.commits_only ? 1u : 0u, a.cm.backlog = backlog ? 1u : 0u;
  a.cm.tiles = a.tiles, a.cm.parts = a.parts;
  a.cm.part = (uint64_t*)(B + o_part), a.cm.sum = (uint64_t*)(B + o_sum);
  ca.part = (uint64_t*)(B + o_cen_part), ca.out = (uint64_t*)(B + o_cen);
  ra.part = (uint64_t*)(B + o_rc_part), ra.out = (uint64_t*)(B + o_rc);
  uint64_t tot[3] = {0, 0, 0};  // the wanted feeds' totals, in the order of their jobs
  if (feeds) {
    JgScanJob jobs[3];
    uint32_t nj = 0;
    uint64_t* const bsum[3] = {a.lw.bsum, a.ir.bsum, a.cm.bsum};
    for (int x = 0; x < 3; x++)
      if (on[x]) jobs[nj++] = JgScanJob{bsum[x], a.tiles, 0};
    HIPCHK(hipMemcpyAsync(B + o_job, jobs, nj * sizeof(JgScanJob), hipMemcpyHostToDevice, e->stream));
    const dim3 grid(a.parts), block(JG_BLOCK);
    // the count pass: ONE over the slots - a single feed's own, else the fused one of the feeds wanted
    if (feeds == 1 && on[POLL_L])
      hipLaunchKernelGGL(k_watch_count, dim3(a.tiles), block, 0, e->stream, e->dev, a.lw);
    else if (feeds == 1 && timed)
      hipLaunchKernelGGL(k_isrc_count, dim3(a.tiles), block, 0, e->stream, e->dev, a.ic);
    else if (feeds == 1 && on[POLL_I])
      hipLaunchKernelGGL(k_isr_count, dim3(a.tiles), block, 0, e->stream, e->dev, a.ir);
    else if (feeds == 1)
      hipLaunchKernelGGL(k_commit_count, grid, block, 0, e->stream, e->dev, a.cm);
    else if (timed && !on[POLL_C])
      hipLaunchKernelGGL((k_poll_count_timed<true, false>), grid, block, 0, e->stream, e->dev, a);
    else if (timed && !on[POLL_L])
      hipLaunchKernelGGL((k_poll_count_timed<false, true>), grid, block, 0, e->stream, e->dev, a);
    else if (timed)
      hipLaunchKernelGGL((k_poll_count_timed<true, true>), grid, block, 0, e->stream, e->dev, a);
    else if (!on[POLL_C])
      hipLaunchKernelGGL((k_poll_count<true, true, false>), grid, block, 0, e->stream, e->dev, a);
    else if (!on[POLL_I])
      hipLaunchKernelGGL((k_poll_count<true, false, true>), grid, block, 0, e->stream, e->dev, a);
    else if (!on[POLL_L])
      hipLaunchKernelGGL((k_poll_count<false, true, true>), grid, block, 0, e->stream, e->dev, a);
    else
      hipLaunchKernelGGL((k_poll_count<true, true, true>), grid, block, 0, e->stream, e->dev, a);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(nj), block, 0, e->stream, (const JgScanJob*)(B + o_job), (uint64_t*)(B + o_total));
    e->n_launch += 2;
    if (backlog) {
      hipLaunchKernelGGL(k_commit_backlog_sum, dim3(1), block, 0, e->stream, a.cm);
      e->n_launch++;
    }
    // (queued unseen: a quiet engine's workgroups return after their two loads)
    if (wcap[POLL_L]) {
      hipLaunchKernelGGL(k_watch_write, dim3(a.tiles), block, 0, e->stream, e->dev, a.lw);
      e->n_launch++;
    }
    if (wcap[POLL_I]) {
      if (timed)
        hipLaunchKernelGGL(k_isrc_write, dim3(a.tiles), block, 0, e->stream, e->dev, a.ic);
      else
        hipLaunchKernelGGL(k_isr_write, dim3(a.tiles), block, 0, e->stream, e->dev, a.ir);
      e->n_launch++;
    }
    if (wcap[POLL_C]) {
      hipLaunchKernelGGL(k_commit_write, dim3(a.tiles), block, 0, e->stream, e->dev, a.cm);
      e->n_launch++;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(tot, B + o_total, nj * 8, hipMemcpyDeviceToHost, e->stream));
    if (backlog) HIPCHK(hipMemcpyAsync(q.backlog, a.cm.sum, JG_CMT_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
  }
  if (census) {
    hipLaunchKernelGGL(k_census, dim3(ca.tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, ca);
    hipLaunchKernelGGL(k_census_sum, dim3(1), dim3(JG_BLOCK), 0, e->stream, ca);
    e->n_launch += 2;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(q.census, ca.out, JG_CENSUS_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
  }
  if (repl) {
    hipLaunchKernelGGL(k_repl_census, dim3(ra.parts), dim3(JG_BLOCK), 0, e->stream, e->dev, ra);
    hipLaunchKernelGGL(k_repl_census_sum, dim3(1), dim3(JG_BLOCK), 0, e->stream, ra);
    e->n_launch += 2;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(q.repl, ra.out, JG_RC_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  const char* const rows[3] = {(const char*)a.lw.out, (const char*)a.ir.out, (const char*)a.cm.out};
  for (int x = 0, j = 0; x < 3; x++) {
    if (!on[x]) continue;
    q.total[x] = (size_t)tot[j++];
    const size_t k = std::min<size_t>(wcap[x], q.total[x]);
    if (k) HIPCHK(hipMemcpy(q.out[x], rows[x], k * POLL_ROW[x], hipMemcpyDeviceToHost));
  }
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_engine_poll(jg_engine* e, jg_poll* p) {
  if (!e || !p) return fail(JG_EINVAL, "null argument");
  const uint32_t all = JG_POLL_LEADERS | JG_POLL_REPLICAS | JG_POLL_COMMITS | JG_POLL_CENSUS | JG_POLL_REPL_CENSUS;
  if (!p->want || (p->want & ~all)) return fail(JG_EINVAL, "jg_engine_poll: want names no part, or an unknown one");
  const bool on[3] = {(p->want & JG_POLL_LEADERS) != 0, (p->want & JG_POLL_REPLICAS) != 0, (p->want & JG_POLL_COMMITS) != 0};
  if (on[POLL_L] && (p->leader_flags & ~(uint32_t)JG_WATCH_PEEK)) return fail(JG_EINVAL, "jg_engine_poll: unknown leader flag");
  if (on[POLL_I] && (p->replica_flags & ~(uint32_t)JG_WATCH_PEEK)) return fail(JG_EINVAL, "jg_engine_poll: unknown replica flag");
  if (on[POLL_C] && (p->commit_flags & ~(uint32_t)(JG_WATCH_PEEK | JG_WATCH_COMMITS_ONLY)))
    return fail(JG_EINVAL, "jg_engine_poll: unknown commit flag");
  const bool timed = on[POLL_I] && p->clock;  // (the clock of a replicas part that is not wanted is not dereferenced)
  const jg_isr_clock clk = timed ? *p->clock : jg_isr_clock{};
  if (timed && clk.now_ms == UINT64_MAX) return fail(JG_EINVAL, "jg_engine_poll: now_ms is UINT64_MAX");
  if (timed && clk.join_lag > clk.caught_lag) return fail(JG_EINVAL, "jg_engine_poll: join_lag above caught_lag");
  if (on[POLL_I] && !timed && p->policy.join_lag > p->policy.leave_lag) return fail(JG_EINVAL, "jg_engine_poll: join_lag above leave_lag");
  if ((on[POLL_L] && p->leaders_cap && !p->leaders) || (on[POLL_I] && p->replicas_cap && !p->replicas) ||
      (on[POLL_C] && p->commits_cap && !p->commits))
    return fail(JG_EINVAL, "jg_engine_poll: null rows with a cap");
  if (((p->want & JG_POLL_CENSUS) && !p->census) || ((p->want & JG_POLL_REPL_CENSUS) && !p->repl_census))
    return fail(JG_EINVAL, "jg_engine_poll: null census");
  if ((uint64_t)p->g0 + p->n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_poll: slot range out of bounds");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  const uint32_t fl[3] = {p->leader_flags, p->replica_flags, p->commit_flags};
  void* const out[3] = {p->leaders, p->replicas, p->commits};
  const size_t cap[3] = {p->leaders_cap, p->replicas_cap, p->commits_cap};
  const bool backlog = on[POLL_C] && p->backlog;
  // what every shard is asked, before its range, its rows and its caps
  PollShard base;
  base.want = p->want;
  for (int x = 0; x < 3; x++) base.peek[x] = (fl[x] & JG_WATCH_PEEK) != 0;
  base.commits_only = (p->commit_flags & JG_WATCH_COMMITS_ONLY) != 0;
  base.pol = p->policy, base.lag_limit = p->census_lag_limit;
  base.timed = timed, base.clk = clk;
  const size_t D = shard_count(e);
  std::vector<PollShard> q(D, base);
  std::vector<uint64_t> w(D * JG_CMT_WORDS, 0);
  std::vector<size_t> at[3];
  if (!e->router) {  // (straight into the caller's arrays; the totals and the gauges only once the call has succeeded)
    PollShard& s = q[0];
    s.g0 = p->g0, s.n = p->n;
    for (int x = 0; x < 3; x++) s.out[x] = out[x], s.cap[x] = cap[x];
    s.backlog = backlog ? w.data() : nullptr;
    if (const int rc = poll_shard(e, s)) return rc;
    for (int x = 0; x < 3; x++) at[x] = {0, s.total[x]};
  } else {
    // a sharded handle: every shard is sized first by ONE fused peek that delivers nothing (the backlog and the censuses
    // are the shards' sums or maxima from that pass); then each shard delivers - and advances - into what is left of EACH
    // feed's own cap behind the shards before it; a shard behind the point where a feed's cap ran out keeps that shadow.
    // Under the time rule the sizing pass keeps the CALLER's peek for the replicas - it delivers nothing (cap 0) and, unless
    // the caller peeks, advances that shard's clocks: time passes on every shard, those behind the cap too; the delivering
    // pass advances them again at the same now_ms, which stores nothing
    int rc = each_shard(e, [&](size_t d) -> int {
      const ShardPart sp = shard_part(e, d, p->g0, p->n);
      PollShard& s = q[d];
      s.g0 = sp.g0, s.n = sp.n;
      for (int x = 0; x < 3; x++) s.peek[x] = x == POLL_I && timed ? base.peek[x] : true;
      s.backlog = backlog ? w.data() + d * JG_CMT_WORDS : nullptr;
      return poll_shard(shard_at(e, d), s);
    });
    if (rc) return rc;
    for (int x = 0; x < 3; x++) {
      at[x].assign(D + 1, 0);
      for (size_t d = 0; d < D; d++) at[x][d + 1] = at[x][d] + q[d].total[x];
    }
    rc = each_shard(e, [&](size_t d) -> int {
      PollShard s = base;
      s.want = 0;
      for (int x = 0; x < 3; x++) {
        if (!on[x] || !cap[x] || !q[d].total[x] || at[x][d] >= cap[x]) continue;
        s.want |= POLL_BIT[x];
        s.out[x] = (char*)out[x] + at[x][d] * POLL_ROW[x], s.cap[x] = cap[x] - at[x][d];
      }
      if (!s.want) return JG_OK;
      s.g0 = q[d].g0, s.n = q[d].n, s.add = e->router->lo[d];
      return poll_shard(shard_at(e, d), s);
    });
    if (rc) return rc;
  }
  if (on[POLL_L]) p->leaders_total = at[POLL_L][D];
  if (on[POLL_I]) p->replicas_total = at[POLL_I][D];
  if (on[POLL_C]) p->commits_total = at[POLL_C][D];
  if (backlog) {
    uint64_t* bw = (uint64_t*)p->backlog;  // (jg_commit_backlog is the backlog words in order: jg_commits.h)
    for (uint32_t x = 0; x < JG_CMT_WORDS; x++) {
      uint64_t t = 0;
      for (size_t d = 0; d < D; d++) t += w[d * JG_CMT_WORDS + x];
      bw[x] = t;
    }
  }
  if (p->want & JG_POLL_CENSUS) {
    uint64_t* o = (uint64_t*)p->census;  // (jg_census is the census words in order: jg_watch.h)
    for (uint32_t x = 0; x < JG_CENSUS_WORDS; x++) {
      uint64_t t = 0;
      for (size_t d = 0; d < D; d++) t = x == JG_CENSUS_MAX_TERM ? std::max(t, q[d].census[x]) : t + q[d].census[x];
      o[x] = t;
    }
  }
  if (p->want & JG_POLL_REPL_CENSUS) {
    uint64_t* o = (uint64_t*)p->repl_census;  // (jg_repl_census is the census words in order: jg_isr.h)
    for (uint32_t x = 0; x < JG_RC_WORDS; x++) {
      uint64_t t = 0;
      for (size_t d = 0; d < D; d++) t = jg_rc_is_max(x) ? std::max(t, q[d].repl[x]) : t + q[d].repl[x];
      o[x] = t;
    }
  }
  return JG_OK;
}

}  // extern "C"
