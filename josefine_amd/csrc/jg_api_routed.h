// jg_api_routed.h - jg_dense_cluster_round_routed: a protocol round with the device-side transport (rows, and the election
// vocabulary as mailbox words).  Part of josefine_gpu.hip's one translation unit.
#pragma once
namespace {
using Route = jg_dense_cluster::Route;
static_assert(JG_MAX_REPLICAS * sizeof(JgApplyJob) <= Route::JOB_SLICE, "job slice too small");
static_assert(JG_MAX_REPLICAS * sizeof(JgFollowerJob) <= Route::JOB_SLICE, "job slice too small");
static_assert(sizeof(JgVoteHalfJobs) + 2 * sizeof(JgVoteMail) <= 4096, "kernel arguments");

// One call of jg_dense_cluster_round_routed, as its phases hand it on.
struct RoutedRound {
  jg_dense_cluster* c = nullptr;
  jg_engine* L = nullptr;  // the lead node: its device and stream carry the round
  uint32_t R = 0;
  uint64_t now_ms = 0;
  const jg_cmd_batch* inject = nullptr;
  // JG_CLUSTER_OPT_VOTE_WORDS (jg_dense_cluster_set_option; jg_votes.h): an election's traffic travels as mailbox words - the campaigns' broadcasts are
  // counted into request words by a census of the emitted rows and are not staged, the answers are written as words by the
  // receiving half (k_vote_half_multi) and never become rows - wherever EVERYTHING a node receives for a partition in a
  // round is such words; every other partition's mail travels as rows, as without the switch.  Fixed for a cluster's life.
  bool vwords = false;
  // which of a node's steps of this round is which PHASE (jg_route.h: the transport orders a partition's mail by phase,
  // emission index, sender): noted as the steps are numbered (note_phase, the one writer)
  std::vector<uint32_t> seq_base, phases;
  // (jobs_v: delivered batches that hold an election's traffic only - the transport's census says so - take the
  // kernel without the chain code: k_apply_vote_runs_multi; jobs_b: the injected rows)
  std::vector<JgApplyJob> jobs_a, jobs_v, jobs_b;
  uint32_t widest_a = 0, widest_v = 0, widest_b = 0;
  std::vector<JgFollowerJob> fjobs;
  // the delivering pass's jobs: every (sender, step) in one launch, every sender's exceptional-row queue in another
  std::vector<JgRouteRecJob> rjobs;
  std::vector<JgRouteXqJob> xjobs;
  size_t rb = 0, xb = 0;  // their bytes in slice 3
  uint32_t widest_r = 0;
  JgVoteHalfJobs vjobs{};  // the vote mail's receiving half on every node (the delivered step's number): kernel arguments
  JgVoteMail vprev{}, vcur{};  // (last round's mail is read, this round's filled)
  // the bucket pass's counters (their size does not depend on the round's rows): cleared with the tallies, in one launch
  JgRouteBuckets bk{};
  uint32_t n_tiles = 0, tile_bits = 0, bk_clear = 0;
  uint32_t ord_bits = 0;  // the emission index's field: the narrow one first, the wide one on a repeat
  size_t words = 0;       // the tallies' (Route::d_count)
  bool cleared = false;   // (the transport's tallies and bucket counters: zeroed with the round's job tables, or by the first attempt's own launch)
  bool ordered = false;   // the ordering pass is queued behind the delivering pass
  uint32_t total = 0, fullest_seg = 0;
  std::vector<uint64_t> to, from;  // rows per destination, per sender
  uint64_t kept = 0, fsm = 0;
  double T0 = 0, T1 = 0, T2 = 0, T3 = 0, T4 = 0;  // JG_TRACE_ROUTE: begun, round issued, delivering pass issued, counts in, done

  // the staging in segments, one cursor each (jg_route_reserve); then the kept exceptional rows per sender
  uint32_t* d_cursor() const { return c->rt.d_count + (size_t)R * ROUTE_WORDS; }
  uint32_t* d_keep_n() const { return d_cursor() + JG_ROUTE_SEGS; }
  const uint32_t* h_cursor() const { return c->rt.h_count + (size_t)R * ROUTE_WORDS; }
  const uint32_t* h_sender(uint32_t s) const { return c->rt.h_count + (size_t)s * ROUTE_WORDS; }
};

size_t route_count_words(uint32_t R) { return (size_t)R * ROUTE_WORDS + JG_ROUTE_SEGS + 2 * R; }
uint32_t route_group_bits(uint32_t G) {
  uint32_t bits = 1;
  while (bits < 32 && (G - 1) >> bits) bits++;
  return bits;
}
// (JG_ROUTE_NARROW_BITS: test hook - a field too narrow for the trace exercises the repeat with the wide one)
uint32_t route_first_ord_bits() {
  static const uint32_t narrow = std::getenv("JG_ROUTE_NARROW_BITS") ? (uint32_t)std::atoi(std::getenv("JG_ROUTE_NARROW_BITS")) : JG_ROUTE_ORD_BITS_FAST;
  return std::min<uint32_t>(std::max<uint32_t>(narrow, 1u), JG_ROUTE_ORD_BITS);
}
// (the job tables of the whole round - both sparse steps, the follower halves, the delivering pass - are written
// first and travel in ONE copy: every table is host bookkeeping only, and a copy costs ~10 us of stream time)
char* route_slice_h(const Route& rt, int k) { return rt.h_jobs + (size_t)k * Route::JOB_SLICE; }
char* route_slice_d(const Route& rt, int k) { return rt.d_jobs + (size_t)k * Route::JOB_SLICE; }
bool run_small_tiles(uint32_t widest) { return widest <= JG_RUN_SMALL_BATCH; }  // (256-row tiles for small batches: four times the workgroups)
uint32_t run_grid(const jg_engine* L, uint32_t widest) {
  const uint32_t tile = run_small_tiles(widest) ? JG_RUN_TILE_SMALL : JG_RUN_TILE;
  return std::min<uint32_t>(std::max<uint32_t>((widest + tile - 1) / tile, 1u), L->count_slots);
}
void note_phase(RoutedRound& s, uint32_t n, uint32_t step, uint32_t phase) {
  if (step < 8) s.phases[n] |= phase << (3u * step);
}
// (the step of node n that has just been numbered)
void note_last_step(RoutedRound& s, uint32_t n, uint32_t phase) { note_phase(s, n, s.c->nodes[n]->seq - s.seq_base[n], phase); }

JgRouteTable route_table(const RoutedRound& s, uint32_t sender) {
  const Route& rt = s.c->rt;
  JgRouteTable t{};
  t.R = s.R, t.src = sender;
  for (uint32_t n = 0; n < s.R; n++) t.member_id[n] = s.c->nodes[n]->cfg.node_ids[n];
  t.src_id = t.member_id[sender];
  t.group_bits = rt.group_bits, t.ord_bits = s.ord_bits, t.cap = rt.cap;
  t.seg_cap = rt.cap / JG_ROUTE_SEGS, t.seg_mask = JG_ROUTE_SEGS - 1;
  t.key = rt.key, t.idx = rt.idx, t.row = rt.row;
  t.cursor = s.d_cursor();
  t.count = rt.d_count + (size_t)sender * ROUTE_WORDS;
  t.kinds = s.d_keep_n() + s.R;
  return t;
}
// the delivering pass's tables into slice 3 (again on a repeated attempt: the table carries the staging's size and the key layout)
int route_jobs(RoutedRound& s) {
  s.rjobs.clear(), s.xjobs.clear(), s.widest_r = 0;
  for (uint32_t n = 0; n < s.R; n++) {
    jg_engine* e = s.c->nodes[n];
    const JgRouteTable t = route_table(s, n);
    for (const StepRec& r : e->recs) {
      if (r.seq <= s.seq_base[n]) continue;
      const uint32_t phase = jg_route_phase(s.phases[n], r.seq - s.seq_base[n]);
      if (!phase) return fail(JG_EDEVICE, "internal: routed round: a step of this round has no phase");  // (the transport would sort its mail first)
      if (!r.d_msg) continue;
      JgRouteRecJob j{};
      j.t = t, j.n = r.n, j.per_row = r.msg_per_row, j.step = phase;
      j.msg_cnt = r.d_msg_cnt, j.msg = r.d_msg, j.fsm_cnt = r.d_fsm_cnt;
      s.rjobs.push_back(j);
      s.widest_r = std::max(s.widest_r, r.n);
    }
    JgRouteXqJob j{};
    j.t = t, j.xq = e->dev.xq, j.xq_n = e->dev.xq_n, j.xq_cap = e->dev.xq_cap, j.seq_base = s.seq_base[n], j.phases = s.phases[n];
    s.xjobs.push_back(j);
  }
  s.rb = s.rjobs.size() * sizeof(JgRouteRecJob), s.xb = s.xjobs.size() * sizeof(JgRouteXqJob);
  if (s.rb + s.xb > Route::JOB_SLICE) return fail(JG_ECAPACITY, "routed round: too many undrained steps for the transport's job table");
  std::memcpy(route_slice_h(s.c->rt, 3), s.rjobs.data(), s.rb);
  std::memcpy(route_slice_h(s.c->rt, 3) + s.rb, s.xjobs.data(), s.xb);
  return JG_OK;
}
// a sparse step of every node that has rows, in one launch: slice 0 the delivered rows - runs of 4-16 rows per group, a RUN
// per lane (jg_apply_runs_body) -, slice 1 the injected ones
int launch_apply(const RoutedRound& s, int slice, const std::vector<JgApplyJob>& jobs, uint32_t widest) {
  if (jobs.empty()) return JG_OK;
  const JgApplyJob* d = (const JgApplyJob*)route_slice_d(s.c->rt, slice);
  if (slice == 0)
    hipLaunchKernelGGL(run_small_tiles(widest) ? k_apply_runs_multi_small : k_apply_runs_multi, dim3(run_grid(s.L, widest), (uint32_t)jobs.size()),
                       dim3(JG_BLOCK), 0, s.L->stream, d);
  else
    hipLaunchKernelGGL(k_apply_rows_multi, dim3(grid_for(widest, s.L->count_slots), (uint32_t)jobs.size()), dim3(JG_BLOCK), 0, s.L->stream, d);
  HIPCHK(hipGetLastError());
  return JG_OK;
}
// The ordering pass: the staged rows in (destination, group, phase, emission index, sender) order -> the command columns of
// every node's next round: bucket by (destination, group tile), sort every bucket in LDS (jg_route.h; round 2's library
// radix sort took 240 us per 1.4 M rows).  (Its counters were cleared with the tallies, before the delivering pass.)
void launch_order(RoutedRound& s, uint32_t fullest_seg) {
  const Route& rt = s.c->rt;
  hipStream_t st = s.L->stream;
  const uint32_t n_seg = JG_ROUTE_SEGS;
  s.bk.shift = s.ord_bits + 3 + JG_ROUTE_STEP_BITS + s.tile_bits;
  const uint32_t seg_cap = rt.cap / n_seg;
  const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>((std::min(fullest_seg, seg_cap) + JG_BLOCK - 1) / JG_BLOCK, 4096 / n_seg));
  hipLaunchKernelGGL(k_route_hist, dim3(grid, n_seg), dim3(JG_BLOCK), 0, st, (const uint32_t*)s.d_cursor(), seg_cap, (const uint64_t*)rt.key, s.bk);
  JgRouteXqDone xd{};  // (the queues the delivering pass delivered whole are emptied by the scan's last workgroup: no launch of their own)
  xd.R = s.R, xd.route_words = ROUTE_WORDS, xd.n_seg = n_seg, xd.seg_cap = seg_cap, xd.count = rt.d_count, xd.cursor = s.d_cursor();
  for (uint32_t n = 0; n < s.R; n++) xd.xq_n[n] = s.c->nodes[n]->dev.xq_n;
  hipLaunchKernelGGL(k_route_scan_all, dim3(s.n_tiles), dim3(JG_BLOCK), 0, st, s.bk, xd);
  hipLaunchKernelGGL(k_route_scatter, dim3(grid, n_seg), dim3(JG_BLOCK), 0, st, (const uint32_t*)s.d_cursor(), seg_cap, (const uint64_t*)rt.key,
                     (const uint32_t*)rt.idx, s.bk, rt.key_alt, rt.idx_alt);
  const uint32_t per_wg = JG_ROUTE_SORT_BUCKETS;
  hipLaunchKernelGGL(k_route_sort_build, dim3((s.bk.n_buckets + per_wg - 1) / per_wg), dim3(JG_BLOCK), 0, st, s.bk, rt.key_alt, rt.idx_alt,
                     (const jg_msg_row*)rt.row, rt.cols, per_wg);
}

// CHECK: everything that refuses the call by its arguments or the cluster's state.  Reads, and changes nothing; after it only
// an allocation or a runtime failure stops the round.
int routed_check(const jg_dense_cluster* c, const jg_cmd_batch* inject) {
  const jg_engine* L = c->nodes[c->lead];
  // (nodes that share a device issue their work on the lead node's stream while clustered: jg_dense_cluster_create)
  for (const jg_engine* e : c->nodes) {
    if (e->device != L->device) return fail(JG_EINVAL, "routed rounds take nodes that share a device");
    if (e->stream != L->stream) return fail(JG_EINVAL, "routed rounds take nodes on the cluster's stream");
    if (!e->p_kind.empty()) return fail(JG_EINVAL, "commands are queued: call jg_step first");
    if (e->inflight.phase) return fail(JG_EINVAL, "a drain is in transfer: jg_drain_flush first");
  }
  if (route_group_bits(c->G) > 29) return fail(JG_EINVAL, "routed rounds: too many groups for the transport's ordering key");
  for (uint32_t n = 0; inject && n < c->R; n++) {
    if (!inject[n].n) continue;
    if (inject[n].n_blocks) return fail(JG_EINVAL, "injected rows cannot carry blocks");
    if (inject[n].n > 0x7fffffffull) return fail(JG_EINVAL, "batch too large: split it");
    if (!inject[n].kind || !inject[n].group || !inject[n].from || !inject[n].term || !inject[n].id || !inject[n].aux || !inject[n].flag)
      return fail(JG_EINVAL, "all seven device columns are required");
  }
  return JG_OK;
}

// PREPARE: what is idempotent and may allocate - every buffer whose size does not depend on the round's rows (the one that
// does, Route::xq_keep[s], stays lazy: routed_settle).  A failure here leaves the cluster as it was: nothing has been consumed.
// Then the record is bound to the buffers.
int routed_prepare(RoutedRound& s) {
  jg_dense_cluster* c = s.c;
  jg_engine* L = s.L;
  Route& rt = c->rt;
  const uint32_t R = s.R;
  int rc = JG_OK;
  for (jg_engine* e : c->nodes)
    if ((rc = ensure_xq(e))) return rc;
  s.words = route_count_words(R);
  if (!rt.d_count) HIPCHK(hipMalloc((void**)&rt.d_count, s.words * 4));
  if (!rt.h_count) HIPCHK(hipHostMalloc((void**)&rt.h_count, s.words * 4, hipHostMallocDefault));
  if (!rt.ready) {
    rt.n_in.assign(R, 0), rt.in_off.assign(R, 0), rt.kinds_in.assign(R, 0);
    rt.xq_keep.assign(R, nullptr);
    rt.group_bits = route_group_bits(c->G);
    // room for a round's worth of rows everywhere, allocated once: 2 rows per partition and node with their output
    // regions (this is a 288 GB device: 640 B per partition and node is 3.2 GB at 5 x 1 M)
    if ((rc = route_grow(rt, (size_t)c->G * 2))) return rc;
    for (jg_engine* e : c->nodes)
      if (e->recs.empty()) HIPCHK(e->arenas[e->cur_arena].reserve((size_t)c->G * 640));
    rt.ready = true;
  }
  if (s.vwords && !rt.vm_mem) {  // the vote mail: two rounds', used in turn
    const size_t RG = (size_t)R * c->G, wd = ((size_t)c->G + 63) / 64;
    const size_t per = RG * sizeof(JgVoteRec) + 2 * R * wd * 8;
    HIPCHK(hipMalloc(&rt.vm_mem, 2 * per));
    HIPCHK(hipMemsetAsync(rt.vm_mem, 0, 2 * per, L->stream));  // (the first round reads the mail of a round that never was: none)
    char* p = (char*)rt.vm_mem;
    for (int k = 0; k < 2; k++) {
      JgVoteMail& m = rt.vm[k];
      m.R = R, m.G = c->G, m.words = (uint32_t)wd;
      m.rec = (JgVoteRec*)p, p += RG * sizeof(JgVoteRec);
      m.rowmail = (uint64_t*)p, p += R * wd * 8;
      m.wordmail = (uint64_t*)p, p += R * wd * 8;
    }
  }
  if (!rt.h_jobs) HIPCHK(hipHostMalloc((void**)&rt.h_jobs, 6 * Route::JOB_SLICE, hipHostMallocDefault));
  if (!rt.d_jobs) HIPCHK(hipMalloc((void**)&rt.d_jobs, 6 * Route::JOB_SLICE));
  JgRouteBuckets& bk = s.bk;
  s.tile_bits = std::min<uint32_t>(JG_ROUTE_TILE_BITS, rt.group_bits);
  bk.n_buckets = R << (rt.group_bits - s.tile_bits);
  s.n_tiles = (bk.n_buckets + JG_ROUTE_SCAN_TILE - 1) / JG_ROUTE_SCAN_TILE;
  const size_t bk_words = (size_t)s.n_tiles * JG_ROUTE_SCAN_TILE + bk.n_buckets + 1 + s.n_tiles + 1;  // hist (whole tiles) | cur | done | tile
  if (!rt.bk_hist) HIPCHK(hipMalloc((void**)&rt.bk_hist, bk_words * 4));
  if (!rt.ev_counts) HIPCHK(hipEventCreateWithFlags(&rt.ev_counts, hipEventDisableTiming));
  bk.hist = rt.bk_hist, bk.cur = bk.hist + (size_t)s.n_tiles * JG_ROUTE_SCAN_TILE, bk.done = bk.cur + bk.n_buckets, bk.tile = bk.done + 1;
  s.bk_clear = s.n_tiles * JG_ROUTE_SCAN_TILE + bk.n_buckets + 1;  // counts, cursors and the scan's ticket
  s.vprev = rt.vm[rt.vm_turn ^ 1u], s.vcur = rt.vm[rt.vm_turn];
  s.ord_bits = route_first_ord_bits();
  s.seq_base.resize(R), s.phases.assign(R, 0);
  for (uint32_t n = 0; n < R; n++) s.seq_base[n] = c->nodes[n]->seq;
  return JG_OK;
}

// NUMBER THE STEPS: from here on the round consumes what the transport delivered (*started: an error marks the cluster failed).
// Host bookkeeping only, but for per-partition leadership's own tables, which travel here: every step of the round gets its
// number and its phase, every launch of the round its job table.
int routed_number_steps(RoutedRound& s, bool* started) {
  *started = true;
  jg_dense_cluster* c = s.c;
  Route& rt = c->rt;
  const uint32_t R = s.R;
  const uint64_t now_ms = s.now_ms;
  int rc = JG_OK;
  // -- 1. what the transport delivered last round, then this round's injected rows (per group: in that order).
  // Nodes that share the lead node's stream take each of the two in ONE launch (k_apply_rows_multi).
  for (uint32_t n = 0; n < R; n++) {
    const bool votes = jg_kinds_within(rt.kinds_in[n], JG_KINDS_ELECTION);
    std::vector<JgApplyJob>& jobs = votes ? s.jobs_v : s.jobs_a;
    uint32_t& widest = votes ? s.widest_v : s.widest_a;
    jg_engine* e = c->nodes[n];
    if (!rt.n_in[n] && !s.vwords) continue;
    e->stepped = true;
    e->seq++;  // (the receiving half of the vote mail is this step too: it has a number on every node)
    note_last_step(s, n, JG_ROUTE_PHASE_DELIVERED);
    if (!rt.n_in[n]) continue;
    const size_t o = rt.in_off[n];
    JgApplyJob j{};
    j.d = e->dev;
    // VoteRequest -> one VoteResponse; VoteResponse -> DROP + Heartbeat on elect() (candidate.rs:108-113): two slots per row
    const bool two = votes && jg_kinds_within(rt.kinds_in[n], (1u << JG_CMD_VOTE_REQUEST) | (1u << JG_CMD_VOTE_RESPONSE));
    if ((rc = prepare_rows(e, rt.n_in[n], rt.cols.group + o, rt.cols.kind + o, rt.cols.from + o, rt.cols.term + o, rt.cols.id + o,
                           rt.cols.aux + o, rt.cols.flag + o, nullptr, nullptr, 0, now_ms, &j.a, two ? 2u : 0u)))
      return rc;
    widest = std::max(widest, j.a.n);
    jobs.push_back(j);
    rt.n_in[n] = 0;
  }
  for (uint32_t n = 0; s.inject && n < R; n++) {
    jg_engine* e = c->nodes[n];
    const jg_cmd_batch& b = s.inject[n];
    if (!b.n) continue;
    e->stepped = true;
    e->seq++;
    note_last_step(s, n, JG_ROUTE_PHASE_INJECTED);
    JgApplyJob j{};
    j.d = e->dev;
    const uint64_t* none = (const uint64_t*)e->d_ones;  // (injected rows carry no blocks: routed_check)
    if ((rc = prepare_rows(e, (uint32_t)b.n, b.group, b.kind, b.from, b.term, b.id, b.aux, b.flag, none, none, 0, now_ms, &j.a))) return rc;
    s.widest_b = std::max(s.widest_b, j.a.n);
    s.jobs_b.push_back(j);
  }
  if (c->any) {
    if ((rc = cluster_tables_any(c, now_ms, false))) return rc;  // (its own copy, behind the sparse steps' tables)
    for (uint32_t n = 0; n < R; n++) {  // (every node's two halves: seq - 1 and seq)
      const uint32_t step = c->nodes[n]->seq - s.seq_base[n];
      note_phase(s, n, step - 1u, JG_ROUTE_PHASE_LEADER), note_phase(s, n, step, JG_ROUTE_PHASE_FOLLOWER);
    }
  } else {
    if ((rc = cluster_follower_jobs(c, now_ms, s.fjobs))) return rc;
    for (uint32_t n = 0; n < R; n++)
      if (n != c->lead) note_last_step(s, n, JG_ROUTE_PHASE_FOLLOWER);
    // (the lead node's leader half is numbered by jg_step_dense_leader inside cluster_round_body: its next step)
    note_phase(s, c->lead, s.L->seq - s.seq_base[c->lead] + 1u, JG_ROUTE_PHASE_LEADER);
  }
  for (uint32_t n = 0; n < R; n++)
    for (const StepRec& r : c->nodes[n]->recs)
      if (r.seq > s.seq_base[n] && r.seq - s.seq_base[n] > 7)
        return fail(JG_ECAPACITY, "routed round: more steps than the transport's ordering key numbers");
  if ((rc = route_jobs(s))) return rc;
  if (s.vwords) {
    for (uint32_t n = 0; n < R; n++) {
      jg_engine* e = c->nodes[n];
      JgVoteHalfJob& j = s.vjobs.j[n];
      j.d = e->dev, j.self = n, j.seq = s.seq_base[n] + 1u, j.step = JG_ROUTE_PHASE_DELIVERED, j.need = R - 1u, j.now = now_ms;
      if (e->seq < j.seq) return fail(JG_EDEVICE, "internal: routed round: the delivered step has no number");
    }
  }
  return JG_OK;
}

// HEAD: the job tables' copy with the tallies' clear, the delivered rows' step (with the vote mail: beside its receiving
// half), the injected rows' step (with the vote mail: beside the clearing of the mail that half has just read).
// (With the vote mail the delivered ROWS are other partitions' than the words', so their step could run BESIDE the receiving
// half on a stream of its own: tried in round 6 and removed - the two cross-queue dependencies cost 12-14 us more than the
// 34 us they hide, profiles/r06/ab_side_stream_sort_buckets.txt.)
int routed_head(RoutedRound& s) {
  jg_dense_cluster* c = s.c;
  jg_engine* L = s.L;
  Route& rt = c->rt;
  const uint32_t R = s.R;
  hipStream_t st = L->stream;
  int rc = JG_OK;
  // slices 0-3 in one copy - by a kernel out of the pinned staging (a copy engine's start-up was the round's largest gap)
  if (!s.jobs_a.empty()) std::memcpy(route_slice_h(rt, 0), s.jobs_a.data(), s.jobs_a.size() * sizeof(JgApplyJob));
  if (!s.jobs_v.empty()) std::memcpy(route_slice_h(rt, 0) + s.jobs_a.size() * sizeof(JgApplyJob), s.jobs_v.data(), s.jobs_v.size() * sizeof(JgApplyJob));
  if (!s.jobs_b.empty()) std::memcpy(route_slice_h(rt, 1), s.jobs_b.data(), s.jobs_b.size() * sizeof(JgApplyJob));
  if (!s.fjobs.empty()) std::memcpy(route_slice_h(rt, 2), s.fjobs.data(), s.fjobs.size() * sizeof(JgFollowerJob));
  const uint32_t n8 = (uint32_t)(4 * Route::JOB_SLICE / 8);
  if (s.vwords) {
    // ... and the tallies with it (until round 6: three launches).  (The mail itself - this round's to fill - was cleared beside
    // the injected rows' step of the round before, where the receiving half had just read it: k_apply_rows_clear_multi below.)
    hipLaunchKernelGGL(k_votes_clear, dim3(32), dim3(JG_BLOCK), 0, st, rt.d_count, (uint32_t)s.words, s.bk.hist, s.bk_clear, (uint64_t*)route_slice_d(rt, 0),
                       (const uint64_t*)route_slice_h(rt, 0), n8);
    s.cleared = true;
  } else {
    hipLaunchKernelGGL(k_copy_words, dim3((n8 + JG_BLOCK - 1) / JG_BLOCK), dim3(JG_BLOCK), 0, st, (uint64_t*)route_slice_d(rt, 0),
                       (const uint64_t*)route_slice_h(rt, 0), n8);
  }
  HIPCHK(hipGetLastError());
  uint32_t n_chunks = 0, vote_grid = 1;  // (a workgroup per chunk of the bitmap; its counter slot is blockIdx.x)
  if (s.vwords) {
    uint32_t slots = L->count_slots;
    for (jg_engine* e : c->nodes) slots = std::min(slots, e->count_slots);
    n_chunks = (s.vprev.words + JG_VOTE_CHUNK - 1) / JG_VOTE_CHUNK;
    vote_grid = std::max(1u, std::min(n_chunks, slots));
  }
  if (s.vwords && !s.jobs_a.empty() && s.jobs_v.empty() && run_small_tiles(s.widest_a)) {
    // the vote mail's receiving half and the delivered rows' step side by side in ONE launch (k_round_head_multi)
    hipLaunchKernelGGL(k_round_head_multi, dim3(std::max(vote_grid, run_grid(L, s.widest_a)), R + (uint32_t)s.jobs_a.size()), dim3(JG_BLOCK), 0, st, s.vjobs, R,
                       s.vprev, s.vcur, (const JgApplyJob*)route_slice_d(rt, 0));
    HIPCHK(hipGetLastError());
  } else {  // rows: always; the vote mail: no rows beside the half, election-only batches, or a batch too wide for the small tile - one behind the other
    if ((rc = launch_apply(s, 0, s.jobs_a, s.widest_a))) return rc;
    if (!s.jobs_v.empty()) {  // (different nodes than jobs_a's: the two launches are independent of each other)
      hipLaunchKernelGGL(run_small_tiles(s.widest_v) ? k_apply_vote_runs_multi_small : k_apply_vote_runs_multi,
                         dim3(run_grid(L, s.widest_v), (uint32_t)s.jobs_v.size()), dim3(JG_BLOCK), 0, st,
                         (const JgApplyJob*)route_slice_d(rt, 0) + s.jobs_a.size());
      HIPCHK(hipGetLastError());
    }
    if (s.vwords) {  // (partitions other than the rows': a partition's mail of a round is words or rows, never both)
      hipLaunchKernelGGL(k_vote_half_multi, dim3(vote_grid, R), dim3(JG_BLOCK), 0, st, s.vjobs, s.vprev, s.vcur);
      HIPCHK(hipGetLastError());
    }
  }
  if (!s.vwords) return launch_apply(s, 1, s.jobs_b, s.widest_b);
  // the injected rows' step with the clearing of the mail the receiving half has just read beside it (the next round's to fill)
  const uint32_t gx = s.jobs_b.empty() ? n_chunks : std::max<uint32_t>(grid_for(s.widest_b, L->count_slots), std::min<uint32_t>(n_chunks, 64u));
  hipLaunchKernelGGL(k_apply_rows_clear_multi, dim3(std::min<uint32_t>(gx, L->count_slots), (uint32_t)s.jobs_b.size() + 1u), dim3(JG_BLOCK), 0, st,
                     (const JgApplyJob*)route_slice_d(rt, 1), (uint32_t)s.jobs_b.size(), s.vprev);
  HIPCHK(hipGetLastError());
  return JG_OK;
}

// DENSE: the dense round; ClientRequests only where the lead node (still) leads
using MaskOffers = InStep;  // (the same guard: a flag that is up for a scope)
int routed_dense(RoutedRound& s) {
  if (s.c->any) return cluster_launch_any(s.c);  // (whoever owns a group reads `offered`: nothing to mask)
  // (its own slot's column holds the offers as they are, and the leader half does not look at a non-leader's -
  // JgLeaderNode::mask_offers; until round 6 a launch of its own wrote a masked copy of the column every round)
  MaskOffers mask(s.L->cluster_mask_offers);
  return cluster_round_body(s.c, s.now_ms, true, false, route_slice_h(s.c->rt, 2), route_slice_d(s.c->rt, 2), &s.fjobs);
}

// TRANSPORT: on the lead node's stream behind everybody's round - the census (vote mail), then the delivering pass until it
// settles: repeated with more staging or the wide emission index when the counts say so (the pass modifies nothing).
// The ordering pass (launch_order) takes everything it needs to know about the round's rows from the device - the segments'
// cursors - so it is launched BEHIND the delivering pass before the host has seen the counts: the host then waits for the
// counts' copy only (an event), with the ordering still queued, and does its bookkeeping and the next round's preparation
// while the device works.  (Waiting first left the device idle for the wake-up and the five launches:
// profiles/r04/ab_route_order.txt.)  A pass that has to be repeated repeats the ordering with it.
int routed_transport(RoutedRound& s) {
  jg_dense_cluster* c = s.c;
  jg_engine* L = s.L;
  Route& rt = c->rt;
  const uint32_t R = s.R, n_seg = JG_ROUTE_SEGS;
  hipStream_t st = L->stream;
  int rc = JG_OK;
  for (uint32_t r = 0; r < R; r++)
    if (r != c->lead && (rc = jg_stream_wait(L, c->nodes[r]))) return rc;
  const bool optimistic = rt.last_total != 0;
  if (s.vwords) {  // the census of everything the round emitted (once: a repeated delivering pass finds it done)
    hipLaunchKernelGGL(k_votes_census_multi, dim3(std::max<uint32_t>((s.widest_r + JG_BLOCK - 1) / JG_BLOCK, 64u), (uint32_t)(s.rjobs.size() + s.xjobs.size())),
                       dim3(JG_BLOCK), 0, st, (const JgRouteRecJob*)route_slice_d(rt, 3), (uint32_t)s.rjobs.size(),
                       (const JgRouteXqJob*)(route_slice_d(rt, 3) + s.rb), s.vcur, R - 1u);
    // (the validation of the copies' counts - a launch of its own until round 6, k_votes_validate - rides on the census:
    // profiles/r06/routed_round_15_launches_ab.txt)
    HIPCHK(hipGetLastError());
  }
  for (int attempt = 0;; attempt++) {  // (repeated once when the staging turns out too small)
    if (!s.cleared) hipLaunchKernelGGL(k_route_clear, dim3(64), dim3(JG_BLOCK), 0, st, rt.d_count, (uint32_t)s.words, s.bk.hist, s.bk_clear);
    s.cleared = false;  // (a repeated attempt clears for itself)
    if (attempt) {  // (every attempt ends with a synchronisation - the counts - so the staging is free again)
      if ((rc = route_jobs(s))) return rc;
      HIPCHK(hipMemcpyAsync(route_slice_d(rt, 3), route_slice_h(rt, 3), s.rb + s.xb, hipMemcpyHostToDevice, st));
    }
    {  // the delivering pass: every sender's sparse steps, every sender's exceptional queue and (words) the answer words that must be rows after all, in ONE launch
      const uint32_t rec_x = (s.widest_r + JG_BLOCK * JG_ROUTE_ITEMS - 1) / (JG_BLOCK * JG_ROUTE_ITEMS);
      // (256 workgroups per queue: a round's queue holds a few ten thousand rows, and every workgroup - busy or not - pays the tally)
      const dim3 grid(std::max<uint32_t>(rec_x, 256u), (uint32_t)(s.rjobs.size() + s.xjobs.size() * (s.vwords ? 2 : 1)));
      const JgRouteRecJob* rj = (const JgRouteRecJob*)route_slice_d(rt, 3);
      const JgRouteXqJob* xj = (const JgRouteXqJob*)(route_slice_d(rt, 3) + s.rb);
      if (s.vwords)
        hipLaunchKernelGGL(k_route_deliver_multi_words, grid, dim3(JG_BLOCK), 0, st, rj, (uint32_t)s.rjobs.size(), xj, (uint32_t)s.xjobs.size(), s.vcur);
      else
        hipLaunchKernelGGL(k_route_deliver_multi, grid, dim3(JG_BLOCK), 0, st, rj, (uint32_t)s.rjobs.size(), xj, (uint32_t)s.xjobs.size());
    }
    HIPCHK(hipGetLastError());
    s.ordered = false;
    // (the counts' copy stays on the round's own stream: on a stream of its own - tried in round 6 - the event that orders it
    // behind the delivering pass costs the round's stream as much as the copy did: 0.379-0.385 against 0.372-0.380 ms per round,
    // profiles/r06/ab_counts_on_a_side_stream.txt)
    HIPCHK(hipMemcpyAsync(rt.h_count, rt.d_count, s.words * 4, hipMemcpyDeviceToHost, st));
    if (optimistic) {
      HIPCHK(hipEventRecord(rt.ev_counts, st));
      launch_order(s, 2 * rt.last_fullest_seg + JG_BLOCK);  // (a round's rows come in the numbers the last round's did; the kernels stride)
      HIPCHK(hipGetLastError());
      s.ordered = true;
    }
    s.T2 = node_clk();
    if (optimistic) HIPCHK(hipEventSynchronize(rt.ev_counts));
    else HIPCHK(hipStreamSynchronize(st));  // (the first round: nothing to size the ordering pass with yet)
    s.T3 = node_clk();
    bool wide = false;  // some group emitted more rows in one step than the narrow index field numbers
    for (uint32_t n = 0; n < R; n++) wide = wide || s.h_sender(n)[R + JG_ROUTE_OVERFLOW];
    uint64_t fullest = 0;  // (a segment that ran over: every segment gets that much room, and the pass is repeated)
    for (uint32_t k = 0; k < n_seg; k++) fullest = std::max<uint64_t>(fullest, s.h_cursor()[k]);
    const bool fits = fullest <= rt.cap / n_seg;
    if (fits && !wide) return JG_OK;
    if (attempt >= 2) return fail(JG_EDEVICE, "internal: routed round: the delivering pass does not settle");
    if (wide) {
      if (s.ord_bits == JG_ROUTE_ORD_BITS) return fail(JG_ECAPACITY, "routed round: a group emitted too many rows in one step");
      s.ord_bits = JG_ROUTE_ORD_BITS;
    }
    if (!fits && (rc = route_grow(rt, fullest * n_seg))) return rc;
  }
}

// SETTLE: the counts are in - what every sender keeps for the host is compacted, the ordering pass is launched if it is not
// queued already, the next round's slices are noted, the nodes' own streams wait, and a sender that left nothing for the host
// has its output regions back without a drain.
int routed_settle(RoutedRound& s, jg_route_stats* stats) {
  jg_dense_cluster* c = s.c;
  jg_engine* L = s.L;
  Route& rt = c->rt;
  const uint32_t R = s.R;
  hipStream_t st = L->stream;
  int rc = JG_OK;
  for (uint32_t k = 0; k < JG_ROUTE_SEGS; k++) s.total += s.h_cursor()[k], s.fullest_seg = std::max(s.fullest_seg, s.h_cursor()[k]);
  s.to.assign(R, 0), s.from.assign(R, 0);
  for (uint32_t n = 0; n < R; n++) {
    const uint32_t* h = s.h_sender(n);
    for (uint32_t d = 0; d < R; d++) s.to[d] += h[d], s.from[n] += h[d];
    s.kept += h[R + JG_ROUTE_KEPT] + h[R + JG_ROUTE_KEPT_XQ];
    s.fsm += h[R + JG_ROUTE_FSM];
  }
  // senders that keep rows for the host: the delivered ones leave their slots / the exceptional queue
  JgWordList emptied{};  // exceptional-row queues that were delivered whole: their counts go to zero in one launch
  for (uint32_t n = 0; n < R; n++) {
    jg_engine* e = c->nodes[n];
    const uint32_t* h = s.h_sender(n);
    if (!s.from[n] && !s.vwords) continue;  // (a sender whose only mail was words' copies: they leave its queue too)
    const JgRouteTable t = route_table(s, n);
    if (h[R + JG_ROUTE_KEPT] || h[R + JG_ROUTE_FSM])  // (its steps stay queued for a drain: without the delivered rows)
      for (const StepRec& r : e->recs) {
        if (r.seq <= s.seq_base[n]) continue;
        hipLaunchKernelGGL(k_route_rec_compact, dim3((r.n + JG_BLOCK - 1) / JG_BLOCK), dim3(JG_BLOCK), 0, st, t, r.n, r.msg_per_row,
                           r.d_msg_cnt, r.d_msg);
        hipLaunchKernelGGL(k_count_block_sums, dim3((r.n + JG_SCAN_TILE - 1) / JG_SCAN_TILE), dim3(JG_BLOCK), 0, st, r.d_msg_cnt,
                           r.d_fsm_cnt, r.n, r.d_bsum_m, r.d_bsum_f);
      }
    const uint32_t kx = h[R + JG_ROUTE_KEPT_XQ];
    if (kx) {
      // (the one allocation behind *started: whether a sender keeps exceptional rows is the round's data)
      if (!rt.xq_keep[n]) HIPCHK(hipMalloc((void**)&rt.xq_keep[n], (size_t)e->dev.xq_cap * sizeof(JgXqRec)));
      hipLaunchKernelGGL(k_route_xq<true>, dim3(256), dim3(JG_BLOCK), 0, st, t, (const JgXqRec*)e->dev.xq, (const uint32_t*)e->dev.xq_n,
                         e->dev.xq_cap, s.seq_base[n], s.phases[n], rt.xq_keep[n], s.d_keep_n() + n);
      HIPCHK(hipMemcpyAsync(e->dev.xq, rt.xq_keep[n], (size_t)kx * sizeof(JgXqRec), hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(e->dev.xq_n, s.d_keep_n() + n, 4, hipMemcpyDeviceToDevice, st));
    } else {
      emptied.p[emptied.n++] = e->dev.xq_n;
    }
  }
  // (a round that has rows to order has emptied them already: the last workgroup of its k_route_scan - JgRouteXqDone)
  if (emptied.n && !s.ordered && !s.total) hipLaunchKernelGGL(k_route_clear_words, dim3(1), dim3(64), 0, st, emptied);
  rt.last_total = s.total, rt.last_fullest_seg = s.fullest_seg;
  if (s.total && !s.ordered) launch_order(s, s.fullest_seg);
  uint32_t off = 0;
  for (uint32_t n = 0; n < R; n++) {
    rt.kinds_in[n] = rt.h_count[(size_t)R * ROUTE_WORDS + JG_ROUTE_SEGS + R + n];
    rt.in_off[n] = off, rt.n_in[n] = (uint32_t)s.to[n];
    off += (uint32_t)s.to[n];
  }
  if (off != s.total) return fail(JG_EDEVICE, "internal: routed round: row counts disagree");
  HIPCHK(hipGetLastError());
  for (uint32_t r = 0; r < R; r++)  // the nodes' next steps come behind the transport
    if (r != c->lead && (rc = jg_stream_wait(c->nodes[r], L))) return rc;
  // a round whose sparse steps left nothing for the host needs no drain: its output regions are released here
  for (uint32_t n = 0; n < R; n++) {
    jg_engine* e = c->nodes[n];
    const uint32_t* h = s.h_sender(n);
    if (h[R + JG_ROUTE_KEPT] || h[R + JG_ROUTE_FSM]) continue;
    while (!e->recs.empty() && e->recs.back().seq > s.seq_base[n]) e->recs.pop_back();
    // (nothing of this round reads those regions any more: the delivering pass has completed, and
    // no compaction pass was launched for this sender)
    if (e->recs.empty()) e->arenas[e->cur_arena].reset();
  }
  if (s.vwords) rt.vm_turn ^= 1u;
  s.T4 = node_clk();
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    for (uint32_t n = 0; n < R; n++) stats->delivered[n] = s.to[n];
    stats->kept = s.kept;
    stats->fsm_rows = s.fsm;
  }
  return JG_OK;
}

int round_routed_impl(jg_dense_cluster* c, uint64_t now_ms, const jg_cmd_batch* inject, jg_route_stats* stats, bool* started) {
  static const bool trace = std::getenv("JG_TRACE_ROUTE") != nullptr;
  RoutedRound s;
  s.c = c, s.L = c->nodes[c->lead], s.R = c->R, s.now_ms = now_ms, s.inject = inject;
  s.vwords = c->rt.vote_words && c->R >= 2;
  int rc = routed_check(c, inject);
  if (rc) return rc;
  HIPCHK(hipSetDevice(s.L->device));
  s.T0 = node_clk();
  if ((rc = routed_prepare(s))) return rc;
  if ((rc = routed_number_steps(s, started)) || (rc = routed_head(s)) || (rc = routed_dense(s))) return rc;
  s.T1 = node_clk();
  if ((rc = routed_transport(s)) || (rc = routed_settle(s, stats))) return rc;
  if (trace)
    std::fprintf(stderr, "[jg route] steps+round issued %.0f us, delivering pass issued %.0f us, wait %.0f us, sort+build issued %.0f us (%u rows)\n",
                 s.T1 - s.T0, s.T2 - s.T1, s.T3 - s.T2, s.T4 - s.T3, s.total);
  return JG_OK;
}
}  // namespace

int jg_dense_cluster_round_routed(jg_dense_cluster* c, uint64_t now_ms, const jg_cmd_batch* inject, jg_route_stats* stats) {
  if (!c) return fail(JG_EINVAL, "null argument");
  // Everything that can be checked is checked, and everything that can be allocated ahead is, before the round begins to
  // consume the rows the transport delivered (routed_number_steps); an error AFTER that (a HIP failure, an internal
  // inconsistency) leaves in-flight messages lost or half-routed: the cluster says so from then on instead of carrying on quietly.
  if (c->failed) return fail(JG_EDEVICE, "jg_dense_cluster_round_routed: an earlier routed round failed half-way: destroy the cluster");
  bool started = false;
  const int rc = round_routed_impl(c, now_ms, inject, stats, &started);
  if (rc && started) c->failed = true;
  return rc;
}
