// jg_api_poll.h - the host path of the three change feeds and the two censuses (jg_watch.h, jg_isr.h, jg_isr_clock.h,
// jg_commits.h, jg_poll.h), and jg_engine_poll: any subset of them for one tick in one call.  The separate calls
// (jg_api_feeds.h) are the same path with one part wanted.  A call that reads, under the rules of jg_api_manage.h: every
// argument of every wanted part checked before anything is queued, refused while kept node steps are outstanding (the
// entry point's part), then poll_handle: JG_NODE_ASYNC steps settled ONCE, only the wanted feeds' shadows and clocks
// allocated, one block of scratch carved from the engine's staging for all parts, ONE count pass (a single feed's own
// kernel, else the fused one), one scan launch, the feeds' own write passes and the census kernels queued back to back,
// the small answers copied asynchronously, ONE synchronisation, then the rows of the feeds that have any.  A multi-device
// handle is served shard by shard: sized, then delivered.  And jg_step_node_polled /
// jg_node_poll_view (ABI v21): the same chain queued BEHIND a kept node step over scratch of the step's own arena, gated on
// the device by the step's general-row count, its header and rows sent home on the step's trip and handed out when the
// step's outbox is viewed (node_poll_tail, node_poll_finish: called by jg_api_node.h).  And jg_step_node_awaited /
// jg_node_await_view (ABI v23), jg_step_node_looked (ABI v25) and jg_step_node_hosted (ABI v26): the one entry point of a kept
// step with attachments - the poll, the completion request of jg_api_await.h, the point query of jg_api_lookup.h, the hosting
// request of jg_api_hosting.h, or any of them together.  Part of josefine_gpu.hip's one translation unit.
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

// One poll's chain of kernels over ONE block of scratch: the offsets are handed out first (poll_plan), the block is whoever
// calls' - the engine's staging for jg_engine_poll, the kept-step set's arena for a polled node step - and bound second
// (poll_bind), then the chain is queued without the host seeing a count (poll_queue).
struct PollPlan {
  bool on[3] = {false, false, false}, census = false, repl = false, backlog = false, timed = false;
  uint32_t feeds = 0, nj = 0;
  uint32_t job_of[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};  // feed x's scan job (the wanted feeds' in order)
  size_t wcap[3] = {0, 0, 0};
  JgPollArgs a{};
  JgCensusArgs ca{};
  JgReplCensusArgs ra{};
  Carve c;
  size_t o_total = 0, o_job = 0, o_sum = 0, o_part = 0, o_cnt[3] = {0, 0, 0}, o_bsum[3] = {0, 0, 0}, o_out[3] = {0, 0, 0};
  size_t o_cen = 0, o_cen_part = 0, o_rc = 0, o_rc_part = 0, o_head = 0;
};

// the feed memory the wanted parts need (zero-filled on the engine's stream; only the wanted feeds': an engine that never
// watches a feed does not pay for it), the launch geometry and the sections of the block; `header`: a section for the
// header block of a polled node step too
int poll_plan(jg_engine* e, const PollShard& q, PollPlan& P, bool header) {
  for (int x = 0; x < 3; x++) P.on[x] = (q.want & POLL_BIT[x]) != 0;
  P.census = (q.want & JG_POLL_CENSUS) != 0, P.repl = (q.want & JG_POLL_REPL_CENSUS) != 0;
  P.backlog = P.on[POLL_C] && q.backlog;
  if (P.on[POLL_L] && !e->watch_shadow)  // (zero: every slot was last reported vacant)
    if (const int rc = dev_alloc(e, &e->watch_shadow, e->cfg.n_groups)) return rc;
  if (P.on[POLL_I] && !e->isr_shadow)  // (zero: no slot was last reported leading)
    if (const int rc = dev_alloc(e, &e->isr_shadow, e->cfg.n_groups)) return rc;
  P.timed = P.on[POLL_I] && q.timed;
  if (P.timed && !e->isr_stamp)  // (the clocks, zero-filled: no member was behind at the last sample)
    if (const int rc = dev_alloc(e, &e->isr_stamp, (size_t)e->cfg.n_replicas * e->cfg.n_groups)) return rc;
  if (P.timed && !e->isr_behind)
    if (const int rc = dev_alloc(e, &e->isr_behind, e->cfg.n_groups)) return rc;
  if (P.on[POLL_C] && !e->commit_shadow)  // (zero: every slot was last delivered at genesis)
    if (const int rc = dev_alloc(e, &e->commit_shadow, e->cfg.n_groups)) return rc;
  JgPollArgs& a = P.a;
  a.tiles = (q.n + JG_POLL_TILE - 1) / JG_POLL_TILE;
  a.parts = std::min<uint32_t>(a.tiles, JG_CMT_PARTS);
  P.ca.g0 = q.g0, P.ca.n = q.n, P.ca.tiles = (q.n + JG_CENSUS_TILE - 1) / JG_CENSUS_TILE;
  P.ra.g0 = q.g0, P.ra.n = q.n, P.ra.lag_limit = q.lag_limit;
  P.ra.tiles = (q.n + JG_REPL_CENSUS_TILE - 1) / JG_REPL_CENSUS_TILE;
  P.ra.parts = std::min<uint32_t>(P.ra.tiles, JG_REPL_CENSUS_PARTS);
  Carve& c = P.c;
  P.o_total = c.sect(3 * 8), P.o_job = c.sect(3 * sizeof(JgScanJob)), P.o_sum = c.sect(JG_CMT_WORDS * 8);
  P.o_part = c.sect(P.backlog ? (size_t)a.parts * JG_CMT_WORDS * 8 : 0);
  for (int x = 0; x < 3; x++) {
    P.wcap[x] = P.on[x] ? std::min<size_t>(q.cap[x], q.n) : 0;
    P.o_cnt[x] = c.sect(P.on[x] ? (size_t)a.tiles * 4 : 0), P.o_bsum[x] = c.sect(P.on[x] ? (size_t)a.tiles * 8 : 0);
    P.o_out[x] = c.sect(P.wcap[x] * POLL_ROW[x]);
    if (P.on[x]) P.job_of[x] = P.nj++;
  }
  P.feeds = P.nj;
  P.o_cen = c.sect(JG_CENSUS_WORDS * 8), P.o_cen_part = c.sect(P.census ? (size_t)P.ca.tiles * JG_CENSUS_WORDS * 8 : 0);
  P.o_rc = c.sect(JG_RC_WORDS * 8), P.o_rc_part = c.sect(P.repl ? (size_t)P.ra.parts * JG_RC_WORDS * 8 : 0);
  if (header) P.o_head = c.sect(JG_PH_WORDS * 8);
  return JG_OK;
}

// the arguments of every pass over block B; `gate`: null, or the device word that makes every part peek (jg_poll.h)
void poll_bind(jg_engine* e, const PollShard& q, PollPlan& P, char* B, const uint32_t* gate) {
  JgPollArgs& a = P.a;
  a.lw.g0 = a.ir.g0 = a.cm.g0 = q.g0, a.lw.n = a.ir.n = a.cm.n = q.n, a.lw.add = a.ir.add = a.cm.add = q.add;
  a.lw.peek = q.peek[POLL_L] ? 1u : 0u, a.ir.peek = q.peek[POLL_I] ? 1u : 0u, a.cm.peek = q.peek[POLL_C] ? 1u : 0u;
  a.lw.gate = a.ir.gate = a.cm.gate = gate;
  a.lw.shadow = e->watch_shadow, a.ir.shadow = e->isr_shadow, a.cm.shadow = e->commit_shadow;
  a.lw.cnt = (uint32_t*)(B + P.o_cnt[POLL_L]), a.ir.cnt = (uint32_t*)(B + P.o_cnt[POLL_I]), a.cm.cnt = (uint32_t*)(B + P.o_cnt[POLL_C]);
  a.lw.bsum = (uint64_t*)(B + P.o_bsum[POLL_L]), a.ir.bsum = (uint64_t*)(B + P.o_bsum[POLL_I]), a.cm.bsum = (uint64_t*)(B + P.o_bsum[POLL_C]);
  a.lw.out = (jg_leader_row*)(B + P.o_out[POLL_L]), a.ir.out = (jg_isr_row*)(B + P.o_out[POLL_I]), a.cm.out = (uint4*)(B + P.o_out[POLL_C]);
  a.lw.cap = P.wcap[POLL_L], a.ir.cap = P.wcap[POLL_I], a.cm.cap = P.wcap[POLL_C];
  a.ir.leave_lag = q.pol.leave_lag, a.ir.join_lag = q.pol.join_lag;
  if (P.timed) {  // (the same feed: the shadow, the scratch and the rows are the lag rule's)
    a.ic.g0 = q.g0, a.ic.n = q.n, a.ic.add = q.add, a.ic.peek = a.ir.peek, a.ic.gate = gate;
    a.ic.now1 = q.clk.now_ms + 1, a.ic.max_behind_ms = q.clk.max_behind_ms, a.ic.caught_lag = q.clk.caught_lag, a.ic.join_lag = q.clk.join_lag;
    a.ic.shadow = e->isr_shadow, a.ic.stamp = e->isr_stamp, a.ic.mask = e->isr_behind;
    a.ic.cnt = a.ir.cnt, a.ic.bsum = a.ir.bsum, a.ic.out = a.ir.out, a.ic.cap = a.ir.cap;
  }
  a.cm.commits_only = q.commits_only ? 1u : 0u, a.cm.backlog = P.backlog ? 1u : 0u;
  a.cm.tiles = a.tiles, a.cm.parts = a.parts;
  a.cm.part = (uint64_t*)(B + P.o_part), a.cm.sum = (uint64_t*)(B + P.o_sum);
  P.ca.part = (uint64_t*)(B + P.o_cen_part), P.ca.out = (uint64_t*)(B + P.o_cen);
  P.ra.part = (uint64_t*)(B + P.o_rc_part), P.ra.out = (uint64_t*)(B + P.o_rc);
}

// the wanted feeds' scan jobs, in the order of their totals
uint32_t poll_jobs(const PollPlan& P, JgScanJob* jobs) {
  uint64_t* const bsum[3] = {P.a.lw.bsum, P.a.ir.bsum, P.a.cm.bsum};
  for (int x = 0; x < 3; x++)
    if (P.on[x]) jobs[P.job_of[x]] = JgScanJob{bsum[x], P.a.tiles, 0};
  return P.nj;
}

// the whole chain on the engine's stream: the count pass, ONE scan launch (`jobs`: where the device reads them; the totals
// land in the block), the backlog sum, the write passes, the census kernels - and with `head` the header block behind them
int poll_queue(jg_engine* e, PollPlan& P, char* B, const JgScanJob* jobs, uint64_t* head, const uint32_t* gate) {
  const JgPollArgs& a = P.a;
  const bool* on = P.on;
  const bool timed = P.timed;
  const dim3 block(JG_BLOCK);
  if (P.feeds) {
    const uint32_t feeds = P.feeds;
    const dim3 grid(a.parts);
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
    hipLaunchKernelGGL(k_scan_block_sums, dim3(P.nj), block, 0, e->stream, jobs, (uint64_t*)(B + P.o_total));
    e->n_launch += 2;
    if (P.backlog) {
      hipLaunchKernelGGL(k_commit_backlog_sum, dim3(1), block, 0, e->stream, a.cm);
      e->n_launch++;
    }
    // (queued unseen: a quiet engine's workgroups return after their two loads)
    if (P.wcap[POLL_L]) {
      hipLaunchKernelGGL(k_watch_write, dim3(a.tiles), block, 0, e->stream, e->dev, a.lw);
      e->n_launch++;
    }
    if (P.wcap[POLL_I]) {
      if (timed)
        hipLaunchKernelGGL(k_isrc_write, dim3(a.tiles), block, 0, e->stream, e->dev, a.ic);
      else
        hipLaunchKernelGGL(k_isr_write, dim3(a.tiles), block, 0, e->stream, e->dev, a.ir);
      e->n_launch++;
    }
    if (P.wcap[POLL_C]) {
      hipLaunchKernelGGL(k_commit_write, dim3(a.tiles), block, 0, e->stream, e->dev, a.cm);
      e->n_launch++;
    }
    HIPCHK(hipGetLastError());
  }
  if (P.census) {
    hipLaunchKernelGGL(k_census, dim3(P.ca.tiles), block, 0, e->stream, e->dev, P.ca);
    hipLaunchKernelGGL(k_census_sum, dim3(1), block, 0, e->stream, P.ca);
    e->n_launch += 2;
    HIPCHK(hipGetLastError());
  }
  if (P.repl) {
    hipLaunchKernelGGL(k_repl_census, dim3(P.ra.parts), block, 0, e->stream, e->dev, P.ra);
    hipLaunchKernelGGL(k_repl_census_sum, dim3(1), block, 0, e->stream, P.ra);
    e->n_launch += 2;
    HIPCHK(hipGetLastError());
  }
  if (head) {
    JgPollHeaderArgs h{};
    h.total = (const uint64_t*)(B + P.o_total);
    for (int x = 0; x < 3; x++) h.job[x] = P.job_of[x], h.cap[x] = P.wcap[x];
    h.backlog = P.backlog ? a.cm.sum : nullptr, h.census = P.census ? P.ca.out : nullptr, h.repl = P.repl ? P.ra.out : nullptr;
    h.gate = gate, h.out = head;
    hipLaunchKernelGGL(k_poll_header, dim3(1), block, 0, e->stream, h);
    e->n_launch++;
    HIPCHK(hipGetLastError());
  }
  return JG_OK;
}

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
  PollPlan P;
  if (const int rc = poll_plan(e, q, P, false)) return rc;
  char* B = nullptr;
  if (const int rc = P.c.on_staging(e, B)) return rc;
  poll_bind(e, q, P, B, nullptr);
  uint64_t tot[3] = {0, 0, 0};  // the wanted feeds' totals, in the order of their jobs
  if (P.feeds) {
    JgScanJob jobs[3];
    const uint32_t nj = poll_jobs(P, jobs);
    HIPCHK(hipMemcpyAsync(B + P.o_job, jobs, nj * sizeof(JgScanJob), hipMemcpyHostToDevice, e->stream));
  }
  if (const int rc = poll_queue(e, P, B, (const JgScanJob*)(B + P.o_job), nullptr, nullptr)) return rc;
  if (P.feeds) HIPCHK(hipMemcpyAsync(tot, B + P.o_total, P.nj * 8, hipMemcpyDeviceToHost, e->stream));
  if (P.backlog) HIPCHK(hipMemcpyAsync(q.backlog, P.a.cm.sum, JG_CMT_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
  if (P.census) HIPCHK(hipMemcpyAsync(q.census, P.ca.out, JG_CENSUS_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
  if (P.repl) HIPCHK(hipMemcpyAsync(q.repl, P.ra.out, JG_RC_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const char* const rows[3] = {(const char*)P.a.lw.out, (const char*)P.a.ir.out, (const char*)P.a.cm.out};
  for (int x = 0; x < 3; x++) {
    if (!P.on[x]) continue;
    q.total[x] = (size_t)tot[P.job_of[x]];
    const size_t k = std::min<size_t>(P.wcap[x], q.total[x]);
    if (k) HIPCHK(hipMemcpy(q.out[x], rows[x], k * POLL_ROW[x], hipMemcpyDeviceToHost));
  }
  return JG_OK;
}

// ---- a poll behind a kept node step (jg_step_node_polled) ---------------------------------------------------------------
// where the device reads the scan jobs and where the header block lands, in the set's pinned words
enum { NODE_POLL_JOB_WORDS = 8, NODE_POLL_PINNED_WORDS = NODE_POLL_JOB_WORDS + JG_PH_WORDS };
static_assert(3 * sizeof(JgScanJob) <= NODE_POLL_JOB_WORDS * 8, "the jobs fit in front of the header");

PollShard node_poll_request(const jg_engine::NodePoll& np) {
  PollShard q;
  q.want = np.want, q.g0 = np.g0, q.n = np.n;
  for (int x = 0; x < 3; x++) q.peek[x] = np.peek[x], q.cap[x] = np.cap[x];
  q.commits_only = np.commits_only, q.pol = np.pol, q.timed = np.timed, q.clk = np.clk, q.lag_limit = np.lag_limit;
  static uint64_t wanted[JG_CMT_WORDS];  // (never written: for a polled step `backlog` only says that the part is wanted)
  q.backlog = np.backlog ? wanted : nullptr;
  return q;
}

// The poll of kept step `o`, queued behind the kernels of that step that are in the stream by now, and its trip home on the
// down stream: the header block as one copy, each feed's rows sized from the polled step finished last (the rest is fetched
// when the step is viewed: node_poll_finish).  Scratch, rows and header are the set's arena's - the engine's staging may be
// carved again by a later call while this answer is still on its way.  `gate`: the step's general-row count on the device
// (its first pass: the poll peeks where that is not zero), or null (the step has no such rows, or this is the pass behind
// its catch-up pass).  Synchronises nothing.
int node_poll_tail(jg_engine* e, jg_engine::NodeOut& o, const uint32_t* gate) {
  jg_engine::NodeStep& nd = e->node;
  jg_engine::NodePoll& np = o.poll;
  if (!np.want || !np.n) return JG_OK;
  const PollShard q = node_poll_request(np);
  PollPlan P;
  if (const int rc = poll_plan(e, q, P, true)) return rc;
  if (!np.scratch) HIPCHK(e->arenas[o.arena].alloc(P.c.at, (void**)&np.scratch));  // (the pass behind the catch-up pass: the same block)
  if (!o.h_poll) {
    HIPCHK(hipHostMalloc((void**)&o.h_poll, NODE_POLL_PINNED_WORDS * 8, hipHostMallocDefault));
    std::memset(o.h_poll, 0, NODE_POLL_PINNED_WORDS * 8);
  }
  char* const B = np.scratch;
  poll_bind(e, q, P, B, gate);
  poll_jobs(P, (JgScanJob*)o.h_poll);
  uint64_t* const head = (uint64_t*)(B + P.o_head);
  if (const int rc = poll_queue(e, P, B, (const JgScanJob*)o.h_poll, head, gate)) return rc;
  HIPCHK(hipEventRecord(o.ev_kernels, e->stream));
  HIPCHK(hipStreamWaitEvent(nd.down, o.ev_kernels, 0));
  HIPCHK(hipMemcpyAsync(o.h_poll + NODE_POLL_JOB_WORDS, head, JG_PH_WORDS * 8, hipMemcpyDeviceToHost, nd.down));
  const char* const rows[3] = {(const char*)P.a.lw.out, (const char*)P.a.ir.out, (const char*)P.a.cm.out};
  for (int x = 0; x < 3; x++) {
    if (!np.redone) {  // (the pass behind the catch-up pass lands where the first one did: its copies may still be in flight)
      const size_t last = nd.poll_guess_known ? nd.poll_guess[x] : P.wcap[x];  // (no polled step finished yet: min(cap, n))
      np.copied[x] = std::min(P.wcap[x], last + last / 32 + 4096);             // (the margin of the fsm rows: node_keep_tail)
    }
    const size_t bytes = np.copied[x] * POLL_ROW[x];
    if (!bytes) continue;
    o.l_poll[x].n = 0;
    HIPCHK(o.l_poll[x].reserve(bytes));
    HIPCHK(hipMemcpyAsync(o.l_poll[x].p, rows[x], bytes, hipMemcpyDeviceToHost, nd.down));
  }
  return JG_OK;
}

// Kept step `o` is being viewed and its outputs have landed: the header block says what each feed delivered - the rows the
// step's own copy did not bring are fetched now - and the answer is what jg_node_poll_view hands out from here on.  Before
// the set's arena starts over.
int node_poll_finish(jg_engine* e, jg_engine::NodeOut& o) {
  jg_engine::NodeStep& nd = e->node;
  jg_engine::NodePoll& np = o.poll;
  jg_node_poll& v = o.poll_view;
  v = jg_node_poll{};
  nd.poll_viewed = (int)(&o - nd.sets);
  if (!np.want) return JG_OK;
  v.want = np.want, v.state = np.redone ? (uint32_t)JG_NODE_POLL_REDONE : 0u;
  if (!np.n) return JG_OK;
  const uint64_t* const h = o.h_poll + NODE_POLL_JOB_WORDS;
  const PollShard q = node_poll_request(np);
  PollPlan P;
  if (const int rc = poll_plan(e, q, P, true)) return rc;
  bool fetched = false;
  size_t given[3];
  for (int x = 0; x < 3; x++) {
    given[x] = (size_t)h[JG_PH_GIVEN + x];
    nd.poll_guess[x] = (size_t)h[JG_PH_TOTAL + x];
    if (given[x] <= np.copied[x]) continue;
    o.l_poll[x].n = np.copied[x] * POLL_ROW[x];  // (what has landed moves along if the buffer grows)
    HIPCHK(o.l_poll[x].reserve(given[x] * POLL_ROW[x]));
    HIPCHK(hipMemcpyAsync(o.l_poll[x].p + np.copied[x] * POLL_ROW[x], np.scratch + P.o_out[x] + np.copied[x] * POLL_ROW[x],
                          (given[x] - np.copied[x]) * POLL_ROW[x], hipMemcpyDeviceToHost, e->stream));
    fetched = true;
  }
  if (fetched) HIPCHK(hipStreamSynchronize(e->stream));
  nd.poll_guess_known = true;
  v.leaders = given[POLL_L] ? (const jg_leader_row*)o.l_poll[POLL_L].p : nullptr;
  v.replicas = given[POLL_I] ? (const jg_isr_row*)o.l_poll[POLL_I].p : nullptr;
  v.commits = given[POLL_C] ? (const jg_commit_row*)o.l_poll[POLL_C].p : nullptr;
  v.leaders_n = given[POLL_L], v.replicas_n = given[POLL_I], v.commits_n = given[POLL_C];
  v.leaders_total = (size_t)h[JG_PH_TOTAL + POLL_L], v.replicas_total = (size_t)h[JG_PH_TOTAL + POLL_I];
  v.commits_total = (size_t)h[JG_PH_TOTAL + POLL_C];
  std::memcpy(&v.backlog, h + JG_PH_BACKLOG, sizeof v.backlog);      // (the structs are the words in order: jg_commits.h, jg_watch.h, jg_isr.h)
  std::memcpy(&v.census, h + JG_PH_CENSUS, sizeof v.census);
  std::memcpy(&v.repl_census, h + JG_PH_REPL, sizeof v.repl_census);
  np.scratch = nullptr;  // (the arena's: gone with it)
  return JG_OK;
}

// jg_engine_poll's own rules for every argument of every wanted part.  `outputs`: the output pointers are part of the call
// (jg_engine_poll) - a polled node step never writes through them and does not look at them
int poll_check(const jg_engine* e, const jg_poll* p, bool outputs) {
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
  if (outputs && ((on[POLL_L] && p->leaders_cap && !p->leaders) || (on[POLL_I] && p->replicas_cap && !p->replicas) ||
                  (on[POLL_C] && p->commits_cap && !p->commits)))
    return fail(JG_EINVAL, "jg_engine_poll: null rows with a cap");
  if (outputs && (((p->want & JG_POLL_CENSUS) && !p->census) || ((p->want & JG_POLL_REPL_CENSUS) && !p->repl_census)))
    return fail(JG_EINVAL, "jg_engine_poll: null census");
  if ((uint64_t)p->g0 + p->n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_poll: slot range out of bounds");
  return JG_OK;
}

// The ONE host path of every watch and census call, behind the caller's own checks and refuse_first: the parts `base` wants
// (want, peeks, rules; its range, rows and caps are filled in here per shard) of the handle's slots [g0, g0 + n).  Per
// wanted feed x the first cap[x] changed rows into out[x] and the number of differing slots into *total[x]; `backlog`
// (null: not wanted), `census` and `repl` are the gauges' words.  The caller's totals and gauges are written only once the
// whole call has succeeded.
int poll_handle(jg_engine* e, const PollShard& base, uint32_t g0, uint32_t n, void* const out[3], const size_t cap[3], size_t* const total[3],
                uint64_t* backlog, uint64_t* census, uint64_t* repl) {
  const bool on[3] = {(base.want & JG_POLL_LEADERS) != 0, (base.want & JG_POLL_REPLICAS) != 0, (base.want & JG_POLL_COMMITS) != 0};
  if (!on[POLL_C]) backlog = nullptr;
  size_t tot[3] = {0, 0, 0};
  uint64_t bw[JG_CMT_WORDS] = {}, cw[JG_CENSUS_WORDS] = {}, rw[JG_RC_WORDS] = {};
  auto fold = [&](const PollShard& s) {  // a shard's sizes and gauges into the handle's
    for (int x = 0; x < 3; x++) tot[x] += s.total[x];
    if (s.backlog) merge_words(bw, s.backlog, JG_CMT_WORDS, summed);
    merge_words(cw, s.census, JG_CENSUS_WORDS, [](uint32_t x) { return x == JG_CENSUS_MAX_TERM; });
    merge_words(rw, s.repl, JG_RC_WORDS, [](uint32_t x) { return jg_rc_is_max(x); });
  };
  if (!e->router) {  // (straight into the caller's arrays, and nothing on the heap: a quiet call is all host overhead)
    uint64_t w[JG_CMT_WORDS];
    PollShard s = base;
    s.g0 = g0, s.n = n;
    for (int x = 0; x < 3; x++) s.out[x] = out[x], s.cap[x] = cap[x];
    s.backlog = backlog ? w : nullptr;
    if (const int rc = poll_shard(e, s)) return rc;
    fold(s);
  } else {
    // a sharded handle: every shard is sized first by ONE fused peek that delivers nothing (the backlog and the censuses
    // are the shards' sums or maxima from that pass); then each shard delivers - and advances - into what is left of EACH
    // feed's own cap behind the shards before it; a shard behind the point where a feed's cap ran out keeps that shadow and,
    // with no feed left to deliver, is not called again.
    // Under the time rule the sizing pass keeps the CALLER's peek for the replicas - it delivers nothing (cap 0) and, unless
    // the caller peeks, advances that shard's clocks: time passes on every shard, those behind the cap too; the delivering
    // pass advances them again at the same now_ms, which stores nothing
    const size_t D = shard_count(e);
    std::vector<PollShard> q(D, base);
    std::vector<uint64_t> w(D * JG_CMT_WORDS, 0);
    int rc = each_shard(e, [&](size_t d) -> int {
      const ShardPart sp = shard_part(e, d, g0, n);
      PollShard& s = q[d];
      s.g0 = sp.g0, s.n = sp.n;
      for (int x = 0; x < 3; x++) s.peek[x] = x == POLL_I && base.timed ? base.peek[x] : true;
      s.backlog = backlog ? w.data() + d * JG_CMT_WORDS : nullptr;
      return poll_shard(shard_at(e, d), s);
    });
    if (rc) return rc;
    std::vector<size_t> at[3];  // where shard d's rows of feed x start among the handle's
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
    for (const PollShard& s : q) fold(s);
  }
  for (int x = 0; x < 3; x++)
    if (on[x]) *total[x] = tot[x];
  if (backlog) std::memcpy(backlog, bw, sizeof bw);
  if (base.want & JG_POLL_CENSUS) std::memcpy(census, cw, sizeof cw);
  if (base.want & JG_POLL_REPL_CENSUS) std::memcpy(repl, rw, sizeof rw);
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_engine_poll(jg_engine* e, jg_poll* p) {
  if (!e || !p) return fail(JG_EINVAL, "null argument");
  if (const int rc = poll_check(e, p, true)) return rc;
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  const bool on[3] = {(p->want & JG_POLL_LEADERS) != 0, (p->want & JG_POLL_REPLICAS) != 0, (p->want & JG_POLL_COMMITS) != 0};
  const uint32_t fl[3] = {p->leader_flags, p->replica_flags, p->commit_flags};
  PollShard base;
  base.want = p->want;
  for (int x = 0; x < 3; x++) base.peek[x] = (fl[x] & JG_WATCH_PEEK) != 0;
  base.commits_only = (p->commit_flags & JG_WATCH_COMMITS_ONLY) != 0;
  base.pol = p->policy, base.lag_limit = p->census_lag_limit;
  base.timed = on[POLL_I] && p->clock;  // (the clock of a replicas part that is not wanted is not dereferenced)
  if (base.timed) base.clk = *p->clock;
  void* const out[3] = {p->leaders, p->replicas, p->commits};
  const size_t cap[3] = {p->leaders_cap, p->replicas_cap, p->commits_cap};
  size_t* const total[3] = {&p->leaders_total, &p->replicas_total, &p->commits_total};
  // (jg_commit_backlog, jg_census and jg_repl_census are their words in order: jg_commits.h, jg_watch.h, jg_isr.h)
  return poll_handle(e, base, p->g0, p->n, out, cap, total, (uint64_t*)p->backlog, (uint64_t*)p->census, (uint64_t*)p->repl_census);
}

int jg_step_node_polled(jg_engine* e, uint64_t now_ms, uint32_t flags, const jg_poll* request) {
  return jg_step_node_awaited(e, now_ms, flags, request, nullptr);
}

int jg_step_node_awaited(jg_engine* e, uint64_t now_ms, uint32_t flags, const jg_poll* request, const jg_node_await_request* await) {
  return jg_step_node_looked(e, now_ms, flags, request, await, nullptr);
}

int jg_step_node_looked(jg_engine* e, uint64_t now_ms, uint32_t flags, const jg_poll* request, const jg_node_await_request* await,
                        const jg_group_set* lookup) {
  return jg_step_node_hosted(e, now_ms, flags, request, await, lookup, nullptr);
}

int jg_step_node_hosted(jg_engine* e, uint64_t now_ms, uint32_t flags, const jg_poll* request, const jg_node_await_request* await,
                        const jg_group_set* lookup, const jg_node_hosting_request* hosting) {
  if (!request && !await && !lookup && !hosting) return jg_step_node(e, now_ms, flags);
  const char* const who = hosting ? "jg_step_node_hosted" : lookup ? "jg_step_node_looked" : await ? "jg_step_node_awaited" : "jg_step_node_polled";
  if (!e) return fail(JG_EINVAL, "null argument");
  if (!(flags & (JG_NODE_LEADER_HALF | JG_NODE_FOLLOWER_HALF)) || (flags & ~127u))
    return fail(JG_EINVAL, std::string(who) + ": flags = JG_NODE_LEADER_HALF and / or JG_NODE_FOLLOWER_HALF [| JG_NODE_TICK] | JG_NODE_ASYNC [| JG_NODE_COMMON_AE] [| JG_NODE_FSM_FUSED] | JG_NODE_KEEP");
  if (e->router) return fail(JG_EINVAL, std::string(who) + ": a polled or awaited step is a shard's (jg_get_shard): JG_NODE_KEEP is per shard");
  if (!(flags & JG_NODE_KEEP) || !(flags & JG_NODE_ASYNC))
    return fail(JG_EINVAL, std::string(who) + ": a poll, a completion request, a lookup and a hosting request travel with a kept step: JG_NODE_ASYNC | JG_NODE_KEEP");
  if (request)
    if (const int rc = poll_check(e, request, false)) return rc;
  jg_engine::NodeAwait aw;  // (*await: copied here; its rows and keys once the step has its set - node_await_stage)
  std::vector<uint64_t> keys;  // (the cancel's keys: copied, sorted, distinct)
  if (await) {
    if (await->n && !await->rows) return fail(JG_EINVAL, "null argument");
    if (!e->await.cap) return fail(JG_EINVAL, "jg_step_node_awaited: no open table (jg_engine_await_open)");
    if (const int rc = await_rows_check(e, await->rows, await->n, who)) return rc;
    if (await->flags & ~(uint32_t)JG_WATCH_PEEK) return fail(JG_EINVAL, "jg_step_node_awaited: unknown flag");
    if (await->want_stats > 1u) return fail(JG_EINVAL, "jg_step_node_awaited: want_stats is 0 or 1");
    if (await->now_ms == UINT64_MAX) return fail(JG_EINVAL, "jg_step_node_awaited: now_ms out of range");
    const size_t bound = node_await_bound(e);
    if (await->n > e->await.cap || bound + await->n > e->await.cap)
      return fail(JG_ECAPACITY, "jg_step_node_awaited: the table is full (by the bound: the outstanding steps' watches have not been viewed)");
    aw.on = true, aw.m = await->n, aw.peek = (await->flags & JG_WATCH_PEEK) != 0, aw.stats = await->want_stats != 0;
    aw.now_ms = await->now_ms, aw.cap = await->cap, aw.bound = bound + await->n;
    if (const int rc = await_keys_check(await->cancel_keys, await->cancel_n, await->cancel_mask, who, keys)) return rc;
    aw.ck = keys.size(), aw.cmask = await->cancel_mask;
  }
  jg_engine::NodeLookup lk;  // (*lookup: copied here; its host list once the step has its set - node_lookup_stage)
  if (lookup)
    if (const int rc = node_lookup_check(e, lookup, lk)) return rc;
  jg_engine::NodeHosting hs;  // (*hosting: copied here; its lists and own slots once the step has its set - node_hosting_stage)
  if (hosting)
    if (const int rc = node_hosting_check(e, hosting, hs)) return rc;
  if (e->inflight.phase) return fail(JG_EINVAL, "a drain is in transfer: jg_drain_wait first");
  jg_engine::NodePoll np;  // (*request and *request->clock: copied here)
  if (request) {
    np.want = request->want, np.g0 = request->g0, np.n = request->n;
    const bool on[3] = {(np.want & JG_POLL_LEADERS) != 0, (np.want & JG_POLL_REPLICAS) != 0, (np.want & JG_POLL_COMMITS) != 0};
    const uint32_t fl[3] = {request->leader_flags, request->replica_flags, request->commit_flags};
    const size_t cap[3] = {request->leaders_cap, request->replicas_cap, request->commits_cap};
    for (int x = 0; x < 3; x++) np.peek[x] = on[x] && (fl[x] & JG_WATCH_PEEK), np.cap[x] = on[x] ? cap[x] : 0;
    np.commits_only = on[POLL_C] && (request->commit_flags & JG_WATCH_COMMITS_ONLY);
    np.backlog = on[POLL_C] && request->backlog;
    np.timed = on[POLL_I] && request->clock;
    if (np.timed) np.clk = *request->clock;
    np.pol = request->policy, np.lag_limit = request->census_lag_limit;
  }
  return node_step(e, now_ms, flags, request ? &np : nullptr, await ? &aw : nullptr, await ? await->rows : nullptr, keys.data(),
                   lookup ? &lk : nullptr, lookup ? lookup->groups : nullptr, hosting ? &hs : nullptr, hosting);
}

int jg_node_await_view(jg_engine* e, jg_node_await* out) {
  if (!e || !out) return fail(JG_EINVAL, "null argument");
  if (e->router) return fail(JG_EINVAL, "jg_node_await_view: an awaited step is a shard's (jg_get_shard)");
  if (e->node.poll_viewed < 0) return fail(JG_EINVAL, "jg_node_await_view: no kept step's outbox has been viewed (or a newer step has claimed its set)");
  *out = e->node.sets[e->node.poll_viewed].await_view;
  return JG_OK;
}

int jg_node_poll_view(jg_engine* e, jg_node_poll* out) {
  if (!e || !out) return fail(JG_EINVAL, "null argument");
  if (e->router) return fail(JG_EINVAL, "jg_node_poll_view: a polled step is a shard's (jg_get_shard)");
  if (e->node.poll_viewed < 0) return fail(JG_EINVAL, "jg_node_poll_view: no kept step's outbox has been viewed (or a newer step has claimed its set)");
  *out = e->node.sets[e->node.poll_viewed].poll_view;
  return JG_OK;
}

}  // extern "C"
