// jg_api_node.h - jg_step_node: the dense kernels behind the Apply surface.  Part of josefine_gpu.hip's one translation unit.
#pragma once
// ---- jg_step_node: a node's whole tick from host rows (jg_node.h) -----------------------------------
namespace {
// one output set's outbox: the device columns and their pinned mirrors (either set, whether or not its steps are kept)
int node_set_ensure(jg_engine* e, jg_engine::NodeOut& o) {
  if (o.ev_out) return JG_OK;
  const size_t G = e->cfg.n_groups, R = e->cfg.n_replicas;
  int rc = dev_alloc(e, &o.o_ae, R * G);
  if (rc || (rc = dev_alloc(e, &o.o_beat, G)) || (rc = dev_alloc(e, &o.o_answer, G)) || (rc = dev_alloc(e, &o.o_hbc, G))) return rc;
  HIPCHK(hipMemsetAsync(o.o_ae, 0xff, std::max<size_t>(R * G * 8, 16), e->stream));  // (the own slot's row is never written: JG_NO_ACK once)
  HIPCHK(hipHostMalloc((void**)&o.h_beat, std::max<size_t>(G * sizeof(jg_leader_beat), 16), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void**)&o.h_ae, std::max<size_t>(R * G * 8, 16), hipHostMallocDefault));
  std::memset(o.h_ae, 0xff, std::max<size_t>(R * G * 8, 16));  // (the own slot's row is not downloaded while it is the same for every group)
  HIPCHK(hipHostMalloc((void**)&o.h_answer, std::max<size_t>(G * 8, 16), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void**)&o.h_hbc, std::max<size_t>(G * 8, 16), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void**)&o.h_nsparse, 16, hipHostMallocDefault));
  std::memset(o.h_nsparse, 0, 16);
  HIPCHK(hipEventCreateWithFlags(&o.ev_out, hipEventDisableTiming));  // (last: what says the set is complete)
  return JG_OK;
}
int node_ensure(jg_engine* e) {
  jg_engine::NodeStep& n = e->node;
  if (n.ready) return JG_OK;
  const size_t G = e->cfg.n_groups, R = e->cfg.n_replicas;
  int rc = JG_OK;
#define A(ptr, cnt) \
  if ((rc = dev_alloc(e, &ptr, (cnt))) != JG_OK) return rc
  A(n.cols.answers, R * G);
  A(n.cols.hbr_commit, R * G);
  A(n.cols.token, G);
  A(n.cols.f_beat, G);
  A(n.cols.f_ae, G);
  A(n.cols.f_leader, G);
  A(n.cols.cls, G);
  A(n.cols.lt_max, G);
  A(n.cols.lt_min, G);
  A(n.cols.lf_max, G);
  A(n.cols.lf_min, G);
  A(n.cols.fsm_delta, G);
  A(n.cols.fsm_prev, G);
  A(n.cols.fsm_mid, G);
  A(n.cols.arr, 2 * R * G);
  A(n.cols.fo, 2 * G);
  A(n.cols.sparse_bits, (G + 63) / 64);
  A(n.d_nsparse, 4);
  if ((rc = node_set_ensure(e, n.cur()))) return rc;  // (the other set: when a step is kept)
  HIPCHK(hipHostMalloc((void**)&n.h_in_answers, std::max<size_t>(R * G * 8, 16), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void**)&n.h_in_hbc, std::max<size_t>(R * G * 8, 16), hipHostMallocDefault));
  HIPCHK(hipEventCreateWithFlags(&n.ev_cols, hipEventDisableTiming));
  while (n.group_bits < 32 && (G - 1) >> n.group_bits) n.group_bits++;
  n.bk_tile_bits = std::min<uint32_t>(JG_ROUTE_TILE_BITS, n.group_bits);
  n.bk_buckets = ((uint32_t)G + (1u << n.bk_tile_bits) - 1u) >> n.bk_tile_bits;
  const uint32_t bk_tiles = (n.bk_buckets + JG_ROUTE_SCAN_TILE - 1) / JG_ROUTE_SCAN_TILE;
  n.bk_words = bk_tiles * JG_ROUTE_SCAN_TILE + n.bk_buckets + bk_tiles + 1;  // hist (whole tiles) | cur | tile
  A(n.bk_mem, n.bk_words);
#if JG_BLOCK == 256
  n.n_tiles = ((uint32_t)G + JGN_TILE - 1u) >> JGN_TILE_BITS;
  A(n.bin_cnt, (size_t)JGN_BIN_WGS * (n.n_tiles + 1u));
  A(n.bin_off, (size_t)n.n_tiles + 3u);
#endif
#undef A
  n.ready = true;
  return JG_OK;
}

// JG_NODE_KEEP: what a set needs beyond its outbox - the pinned words its status snapshot, fsm row count and scan job live in
int node_keep_ensure(jg_engine* e, jg_engine::NodeOut& o) {
  const size_t G = e->cfg.n_groups;
  int rc = node_set_ensure(e, o);
  if (rc) return rc;
  if (!o.h_status) {
    char* m = nullptr;
    HIPCHK(hipHostMalloc((void**)&m, 64, hipHostMallocDefault));
    std::memset(m, 0, 64);
    o.h_status = (uint32_t*)m, o.h_total = (uint64_t*)(m + 32), o.h_job = (JgScanJob*)(m + 48);
    HIPCHK(hipEventCreateWithFlags(&o.ev_early, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&o.ev_kernels, hipEventDisableTiming));
  }
  if (!e->node.down) HIPCHK(hipStreamCreateWithFlags(&e->node.down, hipStreamNonBlocking));
  // room up front for what a kept tick brings home and builds: pinning a 24 MB landing buffer or growing an arena by a
  // 150 MB chunk takes milliseconds each, and the two sets and the queue they trade buffers with would pay them one after
  // the other over the engine's first ticks (one fsm row per partition and step is the steady state's yield)
  const size_t rows = G + G / 32 + 4096;
  if (o.l_fsm.cap < rows) HIPCHK(o.l_fsm.reserve(rows));
  if (e->q_fsm.cap < rows && !e->q_fsm.viewed) HIPCHK(e->q_fsm.reserve(rows));
  const size_t build = (size_t)G * 4 + 2 * (size_t)G * JGN_FSM_ROWS * sizeof(jg_fsm_row) + ((G + JG_SCAN_TILE - 1) / JG_SCAN_TILE) * 8 + 4096;
  for (Arena& ar : e->arenas) HIPCHK(ar.reserve(build));  // (an arena in use is left alone)
  return JG_OK;
}
// hands viewed kept steps' fsm rows to the queue jg_drain_applies reads, the older step's first (a pointer swap when the
// consumer has taken everything before them)
int node_keep_handover(jg_engine* e) {
  jg_engine::NodeStep& nd = e->node;
  for (jg_engine::NodeOut* o : {&nd.sets[nd.newest ^ 1u], &nd.cur()}) {
    if (!o->fsm_landed) continue;
    const int rc = handover(e->q_fsm, o->l_fsm, o->fsm_landed);
    if (rc) return rc;
  }
  return JG_OK;
}
int node_keep_tail(jg_engine* e, uint32_t flags);
int node_keep_finish(jg_engine* e, jg_engine::NodeOut& o);
int node_dense_halves(jg_engine* e, uint64_t now_ms, uint32_t flags, uint32_t col_mask, uint32_t sparse_mode, uint64_t* bytes_down);
int node_general(jg_engine* e, const JgNodeRows& rows, size_t n, size_t nb, uint32_t n_sparse, uint64_t now_ms);
int node_fsm_record(jg_engine* e, StepRec& rec, uint32_t flags);
// (jg_api_poll.h) the poll that travels with a kept step: queued behind its kernels, collected when its outbox is viewed
int node_poll_tail(jg_engine* e, jg_engine::NodeOut& o, const uint32_t* gate);
int node_poll_finish(jg_engine* e, jg_engine::NodeOut& o);
// (jg_api_await.h) the completion request that travels with a kept step: staged at entry, queued behind its kernels (and its
// poll), collected when its outbox is viewed
int node_await_stage(jg_engine::NodeOut& o, const jg_await_row* rows, const uint64_t* keys);
int node_await_tail(jg_engine* e, jg_engine::NodeOut& o, const uint32_t* gate);
int node_await_finish(jg_engine* e, jg_engine::NodeOut& o);
// (jg_api_lookup.h) the point query that travels with a kept step: its list staged at entry, one launch queued behind the
// step's kernels (its poll's and its completion request's), collected when its outbox is viewed
int node_lookup_stage(jg_engine* e, jg_engine::NodeOut& o, const uint32_t* list);
int node_lookup_tail(jg_engine* e, jg_engine::NodeOut& o, const uint32_t* gate);
int node_lookup_finish(jg_engine* e, jg_engine::NodeOut& o);
// (jg_api_hosting.h) the hosting request that travels with a kept step: its lists and own slots staged at entry, its check
// and write passes queued last behind the step's kernels, its verdict collected when the step's outbox is viewed
int node_hosting_stage(jg_engine* e, jg_engine::NodeOut& o, const jg_node_hosting_request* req);
int node_hosting_tail(jg_engine* e, jg_engine::NodeOut& o, const uint32_t* gate);
int node_hosting_finish(jg_engine* e, jg_engine::NodeOut& o);
void groups_rewritten(jg_engine* e, uint32_t own_slots = 0);  // (jg_api_manage.h)

// node_step (or node_settle's catch-up pass) is running: its halves' own node_settle calls are not another caller's
struct InStep {
  bool& f;
  explicit InStep(bool& b) : f(b) { f = true; }
  ~InStep() { f = false; }
};
double node_clk() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One call of node_step, as its phases hand it on.
struct NodeRun {
  uint64_t now_ms = 0;
  uint32_t flags = 0, halves = 0;
  bool async = false, keep = false;  // JG_NODE_ASYNC: no synchronisation inside the step - the general-path row count is looked at when the step is settled
  size_t n = 0, nb = 0;              // the batch: rows, blocks
  uint32_t col_mask = 0;             // the slots whose columns were handed out for this step
  uint32_t both_beats = 0;           // a batch with Heartbeat AND AppendEntries rows: their consistency columns are needed
  bool tiled = false;                // the row passes: tiled or flat
  JgNodeRows rows{};                 // the batch on the device
  uint32_t n_sparse = 0;             // general-path rows (a synchronous step knows)
  size_t fsm_rec_seq = 0;            // the step record of the fsm rows (a step that is not kept)
  uint64_t bytes_up = 0, bytes_down = 0;
  double T0 = 0, T1 = 0, T2 = 0;     // JG_TRACE_NODE: begun, before and after the one synchronisation of a synchronous step
};

// CHECK: everything that refuses the call by its arguments or the engine's state.  Reads, and changes nothing; after it only
// an allocation or a runtime failure stops the step.
int node_check(const jg_engine* e, const NodeRun& s) {
  const jg_engine::NodeStep& nd = e->node;
  if (s.keep && !s.async) return fail(JG_EINVAL, "jg_step_node: JG_NODE_KEEP goes with JG_NODE_ASYNC");
  if (s.keep && (e->pipelined || e->inflight.phase)) return fail(JG_EINVAL, "jg_step_node: JG_NODE_KEEP or jg_drain_prefetch - an engine overlaps its drains one way");
  if (nd.kept_n >= (s.keep ? 2u : 1u)) return fail(JG_EINVAL, "jg_step_node: kept steps are outstanding (JG_NODE_KEEP): jg_node_outbox_view first");
  if (s.n > 0x7fffffffull) return fail(JG_EINVAL, "batch too large: split it");
  if (nd.col_mask && !(s.halves & JG_NODE_LEADER_HALF))  // (never dropped silently: the leader half is what applies them)
    return fail(JG_EINVAL, "jg_step_node: a column was handed out (jg_node_inbox_columns) but the leader half does not run");
  return JG_OK;
}

// PREPARE: what is idempotent and may allocate - the step before is settled (an asynchronous one; a kept one: only its row
// passes are waited for), the sets and the grow-only buffers have their room.  Decides tiled or flat.
int node_prepare(jg_engine* e, NodeRun& s) {
  jg_engine::NodeStep& nd = e->node;
  int rc = node_ensure(e);
  if (rc || (rc = node_settle(e)) || (rc = ensure_xq(e))) return rc;
  if (s.keep) {
    if ((rc = node_keep_ensure(e, nd.sets[0])) || (rc = node_keep_ensure(e, nd.sets[1]))) return rc;
    if ((rc = node_keep_handover(e))) return rc;  // (rows nobody drained since their outbox was viewed: the free set's landing buffer is about to be reused)
  }
  // The row passes, TILED (jg_node.h): the rows binned by tile of 256 partitions, one workgroup per tile with the tile's
  // columns in LDS - prefill, classification and scatter in one kernel, whole lines to and from HBM.  JG_CFG_FLAT_ROW_PASSES
  // (the tests' statement of the tiled passes), a step without rows, or more tiles than the binning's LDS table holds: the
  // flat passes (k_node_prefill + k_node_classify + k_node_route: three random accesses per row and pass).
#if JG_BLOCK == 256
  s.tiled = s.n && !(e->cfg.flags & JG_CFG_FLAT_ROW_PASSES) && nd.n_tiles + 1u <= 16384u;
#endif
  if (nd.sp_cap < s.n) {  // (room for every row on the general path; grow-only, like the pinned columns)
    if (nd.sp_key) HIPCHK(hipFree(nd.sp_key));
    if (nd.sp_idx) HIPCHK(hipFree(nd.sp_idx));
    nd.sp_cap = s.n + s.n / 2;
    HIPCHK(hipMalloc((void**)&nd.sp_key, nd.sp_cap * 8));
    HIPCHK(hipMalloc((void**)&nd.sp_idx, nd.sp_cap * 4));
  }
  if (s.tiled && nd.bin_cap < s.n) {
    if (nd.bin_mem) HIPCHK(hipFree(nd.bin_mem));
    nd.bin_cap = s.n + s.n / 2;
    HIPCHK(hipMalloc((void**)&nd.bin_mem, nd.bin_cap * 41 + 64));
  }
  return JG_OK;
}

// CLAIM (JG_NODE_KEEP): the step takes the free set - the step before, outstanding or not, keeps its own until the step
// after this one - and with a step outstanding the other fault / exceptional-row queues and arena too (what that step's
// kernels appended and allocated is collected when its outbox is viewed).  Whatever leaves node_step before count() gets
// back exactly what was taken.  So at every return: kept_n == the sets with `out`; to_view() is the oldest of them;
// cur_set / cur_arena / dev / d_dev are the ones the newest counted step used.
struct NodeClaim {
  jg_engine* e;
  const bool set, queues;
  uint32_t floor = 0;
  static void other_queues(jg_engine* e) {
    e->cur_set ^= 1, e->cur_arena ^= 1;
    e->dev = dev_for_set(e, e->cur_set), e->d_dev = e->d_dev2[e->cur_set];
  }
  NodeClaim(jg_engine* e_, bool keep) : e(e_), set(keep), queues(keep && e_->node.kept_n) {
    if (set) e->node.newest ^= 1u;
    if (queues) other_queues(e), floor = e->fault_floor[e->cur_set], e->fault_floor[e->cur_set] = e->seq;
  }
  void count() {
    if (set) e->node.cur().out = true, e->node.kept_n++;
    counted = true;
  }
  ~NodeClaim() {
    if (counted) return;
    if (queues) e->fault_floor[e->cur_set] = floor, other_queues(e);
    if (set) e->node.newest ^= 1u;
  }
 private:
  bool counted = false;
};

// UPLOAD, column inbound: the handed-out slots' columns go up as they are (8 bytes per partition and peer instead of two rows)
int node_upload_columns(jg_engine* e, NodeRun& s) {
  jg_engine::NodeStep& nd = e->node;
  const uint32_t G = e->cfg.n_groups, R = e->cfg.n_replicas, col_mask = s.col_mask = nd.col_mask;
  for (uint32_t r = 0; r < R;) {  // (neighbouring slots travel in one copy: a copy costs ~10 us before its first byte)
    if (!((col_mask >> r) & 1u)) {
      r++;
      continue;
    }
    uint32_t r1 = r + 1;
    while (r1 < R && ((col_mask >> r1) & 1u) && (((nd.col_hbc_mask >> r1) & 1u) == ((nd.col_hbc_mask >> r) & 1u))) r1++;
    const size_t at = (size_t)r * G, len = (size_t)(r1 - r) * G * 8;
    HIPCHK(hipMemcpyAsync(nd.cols.answers + at, nd.h_in_answers + at, len, hipMemcpyHostToDevice, e->stream));
    if ((nd.col_hbc_mask >> r) & 1u)
      HIPCHK(hipMemcpyAsync(nd.cols.hbr_commit + at, nd.h_in_hbc + at, len, hipMemcpyHostToDevice, e->stream));
    else
      HIPCHK(hipMemsetAsync(nd.cols.hbr_commit + at, 0, len, e->stream));
    s.bytes_up += len * (((nd.col_hbc_mask >> r) & 1u) ? 2 : 1);
    r = r1;
  }
  if (col_mask) {  // (jg_node_inbox_columns waits for this before it hands the same pinned buffers out again)
    HIPCHK(hipEventRecord(nd.ev_cols, e->stream));
    nd.cols_in_flight = true;
  }
  nd.col_mask = nd.col_hbc_mask = 0;  // (a hand-out covers one step)
  return JG_OK;
}

// UPLOAD, the rows in stream order, straight out of the pinned columns jg_submit (or the caller, in place: jg_submit_reserve)
// filled: one copy per column that is present - an optional column nobody provided is all zeros and is not uploaded at all
// (an AppendResponse row is 18 bytes then, not 34).  `lay`: where the columns are in the image.
int node_upload_rows(jg_engine* e, NodeRun& s, jg_engine::RowLayout& lay) {
  const size_t n = s.n, nb = s.nb;
  const uint32_t R = e->cfg.n_replicas;
  node_row_layout(e, n, nb, lay);
  char* B = nullptr;
  jg_engine::EarlyUpload& u = e->up;
  if (u.last_used >= 0) {  // whoever read the last step's rows (its settling included) is in the stream by now
    HIPCHK(hipEventRecord(u.ev_free[u.last_used], e->stream));
    u.read[u.last_used] = true;
    u.last_used = -1;
  }
  if (u.valid && u.lay.same_batch(lay)) {
    // JG_COL_UPLOAD_NOW: the batch left when it was committed - the kernels wait for its copies, nothing else does
    B = u.buf[u.turn];
    HIPCHK(hipStreamWaitEvent(e->stream, u.ev_up, 0));
    s.bytes_up += n * ((lay.id32 ? 4u : 8u) + 4u + 1u + (lay.has_term ? 8u : 0u) + (lay.has_aux ? 8u : 0u) + (lay.has_from ? 4u : 0u) + (lay.has_flag ? 1u : 0u)) + nb * 16u;
    u.last_used = u.turn;
    u.turn ^= 1;
  } else {
    HIPCHK(e->arenas[e->cur_arena].alloc(lay.bytes, (void**)&B));
    const int rc = upload_node_rows(e, lay, B, e->stream, &s.bytes_up);
    if (rc) return rc;
  }
  u.valid = false;
  JgNodeRows& rows = s.rows;
  rows.n = (uint32_t)n;
  rows.group = (const uint32_t*)(B + lay.o_group), rows.kind = (const uint8_t*)(B + lay.o_kind);
  rows.from = lay.has_from ? (const uint32_t*)(B + lay.o_from) : nullptr, rows.term = lay.has_term ? (const uint64_t*)(B + lay.o_term) : nullptr;
  rows.id = (const uint64_t*)(B + lay.o_id), rows.aux = lay.has_aux ? (const uint64_t*)(B + lay.o_aux) : nullptr;
  rows.flag = lay.has_flag ? (const uint8_t*)(B + lay.o_flag) : nullptr;
  rows.packed = lay.packed ? 1u : 0u, rows.id32 = lay.id32 ? 1u : 0u;
  for (uint32_t r = 0; r < JG_MAX_REPLICAS; r++) rows.ids[r] = r < R ? e->cfg.node_ids[r] : 0u;
  rows.blk_id = (const uint64_t*)(B + lay.o_bid), rows.blk_next = (const uint64_t*)(B + lay.o_bnext), rows.n_blocks = nb;
  return JG_OK;
}

#if JG_BLOCK == 256
extern "C++" template <int RR>
void launch_node_tile(jg_engine* e, const NodeRun& s, const JgNodeBin& bin) {
  jg_engine::NodeStep& nd = e->node;
  if (s.halves & JG_NODE_FOLLOWER_HALF)
    hipLaunchKernelGGL((k_node_tile<RR, true>), dim3(bin.n_tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, nd.cols, bin, e->uniform_self, s.halves,
                       s.both_beats, s.col_mask, nd.sp_key, nd.sp_idx, nd.d_nsparse);
  else
    hipLaunchKernelGGL((k_node_tile<RR, false>), dim3(bin.n_tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, nd.cols, bin, e->uniform_self, s.halves,
                       s.both_beats, s.col_mask, nd.sp_key, nd.sp_idx, nd.d_nsparse);
}
// the tiled row passes: count, scan and scatter the rows into their tiles' bins, then one workgroup per tile
void node_tiled_passes(jg_engine* e, const NodeRun& s, const jg_engine::RowLayout& lay) {
  jg_engine::NodeStep& nd = e->node;
  const JgNodeRows& rows = s.rows;
  JgNodeBin bin{};
  bin.n = (uint32_t)s.n, bin.n_tiles = nd.n_tiles;
  bin.chunk = (uint32_t)(((s.n + JGN_BIN_WGS - 1) / JGN_BIN_WGS + JG_BLOCK - 1) / JG_BLOCK * JG_BLOCK);
  bin.n_wg = (uint32_t)((s.n + bin.chunk - 1) / bin.chunk);
  bin.cnt = nd.bin_cnt, bin.tile_off = nd.bin_off, bin.done = nd.d_nsparse + 1;
  char* m = nd.bin_mem;  // widest first: the 16-byte records, then the optional columns the step has
  const size_t cap = nd.bin_cap;
  bin.rows = rows;
  bin.rows.group = nullptr, bin.rows.kind = nullptr, bin.rows.id = nullptr;  // (in the records)
  bin.rec = (JgNodeBinRec*)m, m += cap * 16;
  bin.rows.term = lay.has_term ? (const uint64_t*)m : nullptr, m += cap * 8;
  bin.rows.aux = lay.has_aux ? (const uint64_t*)m : nullptr, m += cap * 8;
  bin.id_hi = lay.id32 ? nullptr : (uint32_t*)m, m += cap * 4;
  bin.rows.from = lay.has_from ? (const uint32_t*)m : nullptr, m += cap * 4;
  bin.rows.flag = lay.has_flag ? (const uint8_t*)m : nullptr;
  const uint32_t nt1 = bin.n_tiles + 1u, G = e->cfg.n_groups;
  if (nt1 <= 4096u) hipLaunchKernelGGL((k_node_bin_count<4096>), dim3(bin.n_wg), dim3(JG_BLOCK), 0, e->stream, rows, bin, G);
  else hipLaunchKernelGGL((k_node_bin_count<16384>), dim3(bin.n_wg), dim3(JG_BLOCK), 0, e->stream, rows, bin, G);
  hipLaunchKernelGGL(k_node_bin_scan, dim3((nt1 + JG_BLOCK / JGN_BIN_SEGS - 1) / (JG_BLOCK / JGN_BIN_SEGS)), dim3(JG_BLOCK), 0, e->stream, bin);
  if (nt1 <= 4096u) hipLaunchKernelGGL((k_node_bin_scatter<4096>), dim3(bin.n_wg), dim3(JG_BLOCK), 0, e->stream, e->dev, rows, bin);
  else hipLaunchKernelGGL((k_node_bin_scatter<16384>), dim3(bin.n_wg), dim3(JG_BLOCK), 0, e->stream, e->dev, rows, bin);
  switch (e->cfg.n_replicas) {
    case 1: launch_node_tile<1>(e, s, bin); break;
    case 2: launch_node_tile<2>(e, s, bin); break;
    case 3: launch_node_tile<3>(e, s, bin); break;
    case 4: launch_node_tile<4>(e, s, bin); break;
    case 5: launch_node_tile<5>(e, s, bin); break;
    case 6: launch_node_tile<6>(e, s, bin); break;
    case 7: launch_node_tile<7>(e, s, bin); break;
    default: launch_node_tile<8>(e, s, bin); break;
  }
  e->n_launch += 4;
}
#endif

// ROW PASSES: the batch's rows into the columns the halves read, the general path's rows listed and counted; a synchronous
// step waits for the count here and runs that path.  Then the batch is consumed.
int node_row_passes(jg_engine* e, NodeRun& s) {
  jg_engine::NodeStep& nd = e->node;
  jg_engine::NodeOut& o = nd.cur();
  if (!s.tiled)
    hipLaunchKernelGGL(k_node_prefill, dim3(grid_for(e->cfg.n_groups, 4096)), dim3(JG_BLOCK), 0, e->stream, e->dev, nd.cols, e->uniform_self,
                       s.halves & JG_NODE_LEADER_HALF, s.halves & JG_NODE_FOLLOWER_HALF, s.both_beats, s.col_mask);
  if (s.n) {
    jg_engine::RowLayout lay;
    int rc = node_upload_rows(e, s, lay);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(nd.d_nsparse, 0, 8, e->stream));  // (word 0: the general path's rows; word 1: the binning scan's ticket)
#if JG_BLOCK == 256
    if (s.tiled) node_tiled_passes(e, s, lay);
    else
#endif
    {
      const uint32_t rgrid = grid_for(s.n, 4096);
      hipLaunchKernelGGL(k_node_classify, dim3(rgrid), dim3(JG_BLOCK), 0, e->stream, e->dev, nd.cols, s.rows, e->uniform_self,
                         s.halves, s.both_beats, s.col_mask);
      hipLaunchKernelGGL(k_node_route, dim3(rgrid), dim3(JG_BLOCK), 0, e->stream, e->dev, nd.cols, s.rows, e->uniform_self,
                         s.both_beats, nd.sp_key, nd.sp_idx, nd.d_nsparse);
      e->n_launch += 3;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(o.h_nsparse, nd.d_nsparse, 4, hipMemcpyDeviceToHost, e->stream));
    if (s.keep) HIPCHK(hipEventRecord(o.ev_early, e->stream));  // (what the NEXT kept step waits for: the row passes, not the halves or the trip home)
    if (!s.async) {
      // the one synchronisation of a synchronous step: how many rows take the general path sizes that launch
      s.T1 = node_clk();
      HIPCHK(hipStreamSynchronize(e->stream));
      s.T2 = node_clk();
      s.n_sparse = o.h_nsparse[0];
      if (s.n_sparse && (rc = node_general(e, s.rows, s.n, s.nb, s.n_sparse, s.now_ms))) return rc;
    }
    // the pinned columns: the OTHER set from here on (an asynchronous step's uploads may still be reading this one)
    e->p_kind.flip(), e->p_flag.flip(), e->p_group.flip(), e->p_from.flip(), e->p_term.flip(), e->p_id.flip();
    e->p_aux.flip(), e->p_blk_id.flip(), e->p_blk_next.flip();
    e->p_has_from = e->p_has_term = e->p_has_aux = e->p_has_flag = false;
    e->p_kinds_seen = 0;
  }
  e->p_unchecked = e->p_packed = e->p_id32 = false;  // (with or without rows: no format of a batch outlives the step)
  return JG_OK;
}

// TAIL: the fsm_tx rows of the dense halves - a kept step's on their way home behind it (node_keep_tail), else a step
// record of its own (per-group regions; compacted by the drains)
int node_tail(jg_engine* e, NodeRun& s) {
  if (s.keep) return node_keep_tail(e, s.flags);
  StepRec rec;
  rec.n = e->cfg.n_groups, rec.seq = e->seq, rec.msg_per_row = 0, rec.fsm_per_row = JGN_FSM_ROWS;
  Arena& ar = e->arenas[e->cur_arena];
  HIPCHK(ar.alloc((size_t)rec.n * 4, (void**)&rec.d_fsm_cnt));
  HIPCHK(ar.alloc((size_t)rec.n * JGN_FSM_ROWS * sizeof(jg_fsm_row), (void**)&rec.d_fsm));
  HIPCHK(ar.alloc((size_t)((rec.n + JG_SCAN_TILE - 1) / JG_SCAN_TILE) * 8, (void**)&rec.d_bsum_f));
  const int rc = node_fsm_record(e, rec, s.flags);
  if (rc) return rc;
  e->recs.push_back(rec);
  s.fsm_rec_seq = rec.seq;
  return JG_OK;
}
// (the one launch that fills a step record's fsm regions: the step's, and once more from node_settle's catch-up pass)
int node_fsm_record(jg_engine* e, StepRec& rec, uint32_t flags) {
  const uint32_t n_tiles = (e->cfg.n_groups + JG_SCAN_TILE - 1) / JG_SCAN_TILE;
  hipLaunchKernelGGL(k_node_fsm_build, dim3(n_tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, e->node.cols, rec.d_fsm, rec.d_fsm_cnt, rec.d_bsum_f,
                     (flags & JG_NODE_FSM_FUSED) ? 1u : 0u);
  HIPCHK(hipGetLastError());
  e->n_launch++;
  return JG_OK;
}

// PUBLISH: the step is what the next view, settle and step find.  A kept step is counted here (NodeClaim::count).
int node_publish(jg_engine* e, const NodeRun& s, uint32_t seq0, NodeClaim& claim) {
  jg_engine::NodeStep& nd = e->node;
  jg_engine::NodeOut& o = nd.cur();
  HIPCHK(hipEventRecord(o.ev_out, s.keep ? nd.down : e->stream));  // (a kept step: everything of it that travels home is on the down stream, behind its kernels)
  o.seq_hi = e->seq;
  claim.count();
  jg_engine::NodePending& pend = o.pending;
  pend = jg_engine::NodePending{};
  pend.rows = s.rows, pend.n = s.n, pend.nb = s.nb, pend.fsm_rec_seq = s.fsm_rec_seq;
  pend.now_ms = s.now_ms, pend.flags = s.flags, pend.col_mask = s.col_mask;
  pend.seq_general = seq0 + 1, pend.seq_end = e->seq;
  pend.on = s.async && s.n != 0;  // (nothing is pending when there were no rows: no general path to come back for)
  o.last = jg_node_outbox{};
  o.last.rows = s.n, o.last.rows_general = s.n_sparse, o.last.bytes_h2d = s.bytes_up, o.last.bytes_d2h = s.bytes_down;
  o.last_flags = s.flags;
  return JG_OK;
}

// `poll`: the request of a polled step (jg_step_node_polled: checked, and a kept step's), or null; `await`: the completion
// request of an awaited step (jg_step_node_awaited: checked, its bound taken), the rows it registers and the keys it cancels
// (aw.ck of them: sorted, distinct), or null; `lookup`: the point query of a looked step (jg_step_node_looked: checked) and
// its host list (lookup->listed), or null; `hosting`: the hosting request of a hosted step (jg_step_node_hosted: checked) and
// the caller's two sets, whose lists and own slots are copied here, or null
int node_step(jg_engine* e, uint64_t now_ms, uint32_t flags, const jg_engine::NodePoll* poll, const jg_engine::NodeAwait* await,
              const jg_await_row* await_rows, const uint64_t* await_keys, const jg_engine::NodeLookup* lookup, const uint32_t* lookup_list,
              const jg_engine::NodeHosting* hosting, const jg_node_hosting_request* hosting_req) {
  static const bool trace = std::getenv("JG_TRACE_NODE") != nullptr;
  jg_engine::NodeStep& nd = e->node;
  NodeRun s;
  s.now_ms = now_ms, s.flags = flags, s.halves = flags & (JG_NODE_LEADER_HALF | JG_NODE_FOLLOWER_HALF);
  s.async = (flags & JG_NODE_ASYNC) != 0, s.keep = (flags & JG_NODE_KEEP) != 0;
  s.n = e->p_kind.size(), s.nb = e->p_blk_id.size();
  s.both_beats = (e->p_kinds_seen & 3u) == 3u;
  s.T0 = s.T1 = s.T2 = node_clk();
  HIPCHK(hipSetDevice(e->device));
  int rc = node_check(e, s);
  if (rc || (rc = node_prepare(e, s))) return rc;
  NodeClaim claim(e, s.keep);  // (from here on nd.cur() is this step's set)
  jg_engine::NodeOut& o = nd.cur();
  o.keep = s.keep, o.pending.on = false;
  if (nd.poll_viewed == (int)nd.newest) nd.poll_viewed = -1;  // (the answer viewed last lived in this set)
  o.poll = poll ? *poll : jg_engine::NodePoll{};
  o.aw = await ? *await : jg_engine::NodeAwait{};
  if (o.aw.on && (rc = node_await_stage(o, await_rows, await_keys))) return rc;  // (the rows are the caller's until here)
  o.lk = lookup ? *lookup : jg_engine::NodeLookup{};
  if (o.lk.on && (rc = node_lookup_stage(e, o, lookup_list))) return rc;  // (... and the list)
  o.hs = hosting ? *hosting : jg_engine::NodeHosting{};
  if (o.hs.on && (rc = node_hosting_stage(e, o, hosting_req))) return rc;  // (... and the two sets' lists and own slots)
  o.hs.now = now_ms, o.hs.self0 = e->uniform_self;
  if (s.keep) {  // (the set starts empty: its last step's regions went with that step's arena)
    o.set = e->cur_set, o.arena = e->cur_arena, o.irr_gen = e->irr_gen;
    o.d_fsm_cnt = nullptr, o.d_fsm = o.d_stage = nullptr, o.d_bsum = nullptr;
    o.fsm_copied = 0, o.l_fsm.n = 0;
  }
  e->stepped = true;
  InStep in_step(nd.in_step);
  // the general path's sequence number is taken whether or not it runs: the shards of a multi-device engine must leave
  // one node step with the same numbers (the router merges their rows by step number first: jg_multi.h)
  const uint32_t seq0 = e->seq;
  if ((rc = node_upload_columns(e, s))) return rc;
  e->seq = seq0 + 1;
  if ((rc = node_row_passes(e, s))) return rc;
  // the dense halves: every partition, the ones whose rows went the general way included (they are ticked here) -
  // except in an asynchronous step, whose halves leave those partitions to the catch-up pass (node_settle)
  e->seq = seq0 + 1;  // (the halves number themselves from the general path's number, whether or not it ran)
  if ((rc = node_dense_halves(e, now_ms, flags, s.col_mask, s.async && s.n ? 1u : 0u, &s.bytes_down))) return rc;
  if ((rc = node_tail(e, s))) return rc;
  // the poll behind the step: gated by the step's own general-row count, final once the route pass has run (no rows: no gate)
  if (o.poll.want && (rc = node_poll_tail(e, o, s.n ? nd.d_nsparse : nullptr))) return rc;
  if (o.aw.on && (rc = node_await_tail(e, o, s.n ? nd.d_nsparse : nullptr))) return rc;
  if (o.lk.on && (rc = node_lookup_tail(e, o, s.n ? nd.d_nsparse : nullptr))) return rc;
  // the hosting pass is the last thing behind the step: whatever the step itself answers has seen the engine without it
  if (o.hs.on && (rc = node_hosting_tail(e, o, s.n ? nd.d_nsparse : nullptr))) return rc;
  if ((rc = node_publish(e, s, seq0, claim))) return rc;
  // what a rewrite of group state owes the engine's summaries of it, from the NEXT step on: this step's status block was
  // taken before the pass and its irr_gen at the claim, so it settles no flag; its catch-up pass assumes o.hs.self0.
  // (Conservative where the device refuses a set: the host cannot know yet.)
  if (o.hs.on && (o.hs.close.n || o.hs.open.n)) groups_rewritten(e, o.hs.own_mask);
  if (trace)
    std::fprintf(stderr, "[jg node] %zu rows: uploads + classify + route issued in %.0f us, waited %.0f us (H2D %.1f MB), halves + fsm build + outbox copies issued in %.0f us\n",
                 s.n, s.T1 - s.T0, s.T2 - s.T1, s.bytes_up / 1e6, node_clk() - s.T2);
  return JG_OK;
}

// a set's AppendEntries words by addressee, on their way home: every slot's row but the own one's (JG_NO_ACK on both sides
// and stays there: not written, not downloaded)
int node_fetch_ae_rows(jg_engine* e, jg_engine::NodeOut& o, hipStream_t st, uint64_t* bytes) {
  const uint32_t G = e->cfg.n_groups, R = e->cfg.n_replicas, own = e->uniform_self >= 0 ? (uint32_t)e->uniform_self : R;
  if (own > 0) HIPCHK(hipMemcpyAsync(o.h_ae, o.o_ae, (size_t)std::min(own, R) * G * 8, hipMemcpyDeviceToHost, st));
  if (own + 1 < R)
    HIPCHK(hipMemcpyAsync(o.h_ae + (size_t)(own + 1) * G, o.o_ae + (size_t)(own + 1) * G, (size_t)(R - own - 1) * G * 8, hipMemcpyDeviceToHost, st));
  *bytes += (size_t)G * (size_t)(own < R ? R - 1 : R) * 8;
  return JG_OK;
}
// The dense halves of a node step + the downloads of their outbox columns.  sparse_mode: 0 every partition; 1 all but
// the partitions whose rows take the general path (an asynchronous step, first pass); 2 only those (its catch-up pass).
int node_dense_halves(jg_engine* e, uint64_t now_ms, uint32_t flags, uint32_t col_mask, uint32_t sparse_mode, uint64_t* bytes_down) {
  jg_engine::NodeStep& nd = e->node;
  jg_engine::NodeOut& o = nd.cur();
  const uint32_t halves = flags & (JG_NODE_LEADER_HALF | JG_NODE_FOLLOWER_HALF);
  const bool tick = (flags & JG_NODE_TICK) != 0;
  const uint32_t G = e->cfg.n_groups;
  int rc = JG_OK;
  // where the outbox columns travel home: a kept step's on the down stream, behind the kernels that wrote them
  hipStream_t ds = o.keep ? nd.down : e->stream;
  auto behind_the_kernels = [&]() -> hipError_t {
    if (!o.keep) return hipSuccess;
    hipError_t err = hipEventRecord(o.ev_kernels, e->stream);
    return err != hipSuccess ? err : hipStreamWaitEvent(nd.down, o.ev_kernels, 0);
  };
  if (halves & JG_NODE_LEADER_HALF) {
    JgLeaderNode ln{};
    ln.hbr_commit = nd.cols.hbr_commit;
    ln.packed = 1;
    ln.ack_stride = 1;
    const bool common = tick && (flags & JG_NODE_COMMON_AE);
    if (common && !o.o_aec && (rc = dev_alloc(e, &o.o_aec, (size_t)G))) return rc;
    if (common && !o.h_aec) HIPCHK(hipHostMalloc((void**)&o.h_aec, std::max<size_t>((size_t)G * 8, 16), hipHostMallocDefault));  // (per set: JG_NODE_KEEP)
    if (tick) ln.o_beat = o.o_beat, ln.o_ae = o.o_ae;
    if (common) ln.o_aec = o.o_aec;
    ln.now = now_ms;
    ln.fsm_delta = nd.cols.fsm_delta, ln.fsm_prev = nd.cols.fsm_prev, ln.fsm_mid = nd.cols.fsm_mid;
    ln.arr = nd.cols.arr, ln.col_mask = col_mask;  // (the slow kernel replays its groups in arrival order)
    if (sparse_mode) ln.sparse_bits = nd.cols.sparse_bits, ln.sparse_mode = sparse_mode;
    if ((rc = dense_step(e, nd.cols.answers, 1, &ln))) return rc;
    if (common) {
      // one word per partition; the rows only if some partition's words differ by addressee (fetched by
      // jg_node_outbox_view, which sees the count: none in the steady state)
      HIPCHK(hipMemsetAsync(nd.d_nsparse + 2, 0, 4, e->stream));
      hipLaunchKernelGGL(k_node_count_individual, dim3(grid_for(G, 1024)), dim3(JG_BLOCK), 0, e->stream, (const uint64_t*)o.o_aec, G, nd.d_nsparse + 2);
      HIPCHK(hipGetLastError());
      e->n_launch++;
      HIPCHK(hipMemcpyAsync(o.h_nsparse + 2, nd.d_nsparse + 2, 4, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(behind_the_kernels());
      HIPCHK(hipMemcpyAsync(o.h_beat, o.o_beat, (size_t)G * sizeof(jg_leader_beat), hipMemcpyDeviceToHost, ds));
      HIPCHK(hipMemcpyAsync(o.h_aec, o.o_aec, (size_t)G * 8, hipMemcpyDeviceToHost, ds));
      o.ae_rows_landed = false;
      *bytes_down += (size_t)G * (sizeof(jg_leader_beat) + 8) + 4;
    } else if (tick) {
      o.ae_rows_landed = true;
      HIPCHK(behind_the_kernels());
      HIPCHK(hipMemcpyAsync(o.h_beat, o.o_beat, (size_t)G * sizeof(jg_leader_beat), hipMemcpyDeviceToHost, ds));
      if ((rc = node_fetch_ae_rows(e, o, ds, bytes_down))) return rc;
      *bytes_down += (size_t)G * sizeof(jg_leader_beat);
    }
  }
  if (halves & JG_NODE_FOLLOWER_HALF) {
    jg_follower_inbox fi{};
    fi.leader = nd.cols.f_leader, fi.beat = nd.cols.f_beat, fi.ae = nd.cols.f_ae;
    const jg_follower_outbox fo{o.o_answer, o.o_hbc};
    if ((rc = follower_half(e, now_ms, &fi, &fo, tick ? 1 : 0, nd.cols.fsm_delta, nd.cols.fsm_prev,
                            sparse_mode ? nd.cols.sparse_bits : nullptr, sparse_mode)))
      return rc;
    HIPCHK(behind_the_kernels());
    HIPCHK(hipMemcpyAsync(o.h_answer, o.o_answer, (size_t)G * 8, hipMemcpyDeviceToHost, ds));
    HIPCHK(hipMemcpyAsync(o.h_hbc, o.o_hbc, (size_t)G * 8, hipMemcpyDeviceToHost, ds));
    *bytes_down += (size_t)G * 16;
  }
  return JG_OK;
}

// The general path of a node step: the rows k_node_route listed (in no particular order) are put into group-major
// order, a group's rows in the order they arrived, by the bucket pass of jg_route.h - key = group << 32 | arrival index,
// a bucket = 256 groups, one workgroup ranks a bucket - and become the batch k_apply_rows takes: exactly jg_submit +
// jg_step for those partitions, in stream order.  (Round 3: rocprim::select + radix_sort_pairs.)
int node_general(jg_engine* e, const JgNodeRows& rows, size_t n, size_t nb, uint32_t n_sparse, uint64_t now_ms) {
  jg_engine::NodeStep& nd = e->node;
  Arena& ar = e->arenas[e->cur_arena];
  (void)n;
  uint64_t* key_alt = nullptr;
  uint32_t *idx_alt = nullptr, *order = nullptr;
  HIPCHK(ar.alloc((size_t)n_sparse * 8, (void**)&key_alt));
  HIPCHK(ar.alloc((size_t)n_sparse * 4, (void**)&idx_alt));
  HIPCHK(ar.alloc((size_t)n_sparse * 4, (void**)&order));
  JgRouteBuckets bk{};
  bk.n_buckets = nd.bk_buckets, bk.shift = 32 + nd.bk_tile_bits;
  const uint32_t bk_tiles = (bk.n_buckets + JG_ROUTE_SCAN_TILE - 1) / JG_ROUTE_SCAN_TILE;
  bk.hist = nd.bk_mem, bk.cur = bk.hist + (size_t)bk_tiles * JG_ROUTE_SCAN_TILE, bk.tile = bk.cur + bk.n_buckets;
  hipStream_t st = e->stream;
  hipLaunchKernelGGL(k_route_clear, dim3(64), dim3(JG_BLOCK), 0, st, bk.hist, bk_tiles * JG_ROUTE_SCAN_TILE + bk.n_buckets, bk.tile, bk_tiles + 1);
  const uint32_t grid = std::min<uint32_t>((n_sparse + JG_BLOCK - 1) / JG_BLOCK, 4096);
  hipLaunchKernelGGL(k_route_hist, dim3(grid, 1), dim3(JG_BLOCK), 0, st, (const uint32_t*)nd.d_nsparse, (uint32_t)nd.sp_cap, (const uint64_t*)nd.sp_key, bk);
  hipLaunchKernelGGL(k_route_scan, dim3(bk_tiles), dim3(JG_BLOCK), 0, st, bk);
  hipLaunchKernelGGL(k_route_scan_tiles, dim3(1), dim3(JG_BLOCK), 0, st, bk);
  hipLaunchKernelGGL(k_route_scatter, dim3(grid, 1), dim3(JG_BLOCK), 0, st, (const uint32_t*)nd.d_nsparse, (uint32_t)nd.sp_cap, (const uint64_t*)nd.sp_key,
                     (const uint32_t*)nd.sp_idx, bk, key_alt, idx_alt);
  hipLaunchKernelGGL(k_bucket_order, dim3(bk.n_buckets), dim3(JG_BLOCK), 0, st, bk, (const uint64_t*)key_alt, (const uint32_t*)idx_alt, order);
  const uint32_t sgrid = (n_sparse + JG_BLOCK - 1) / JG_BLOCK;
  JgNodeSorted so{};
  char* M = nullptr;
  const size_t ns = n_sparse;
  HIPCHK(ar.alloc(ns * 34 + 64, (void**)&M));  // 3 x 8 + 2 x 4 + 2 x 1 bytes per row, widest columns first
  so.term = (uint64_t*)M, M += ns * 8;
  so.id = (uint64_t*)M, M += ns * 8;
  so.aux = (uint64_t*)M, M += ns * 8;
  so.group = (uint32_t*)M, M += ns * 4;
  so.from = (uint32_t*)M, M += ns * 4;
  so.kind = (uint8_t*)M, M += ns;
  so.flag = (uint8_t*)M;
  hipLaunchKernelGGL(k_node_gather_rows, dim3(sgrid), dim3(JG_BLOCK), 0, st, n_sparse, (const uint32_t*)order, rows, so);
  HIPCHK(hipGetLastError());
  e->n_launch += 7;
  return launch_rows(e, n_sparse, so.group, so.kind, so.from, so.term, so.id, so.aux, so.flag,
                     nb ? rows.blk_id : (const uint64_t*)e->d_ones, nb ? rows.blk_next : (const uint64_t*)e->d_ones, nb, now_ms);
}

// An asynchronous node step is settled the first time anything looks at the engine again: the general-path row count
// has landed by then; if it is not zero, those rows are applied now (their sequence number was reserved) and the dense
// halves come back for exactly the partitions they left alone - same results, same record order, one pass later.
int node_settle(jg_engine* e) {
  jg_engine::NodeStep& nd = e->node;
  if (nd.in_step) return JG_OK;  // (the halves of the step that is running)
  jg_engine::NodeOut& o = nd.cur();
  jg_engine::NodePending& pd = o.pending;
  if (!pd.on) return JG_OK;
  pd.on = false;
  HIPCHK(hipSetDevice(e->device));
  // (a kept step: its row passes are what the count depends on - the halves, the fsm rows and the trip home go on)
  if (o.keep) HIPCHK(hipEventSynchronize(o.ev_early));
  else HIPCHK(hipStreamSynchronize(e->stream));
  const uint32_t n_sparse = o.h_nsparse[0];
  o.last.rows_general = n_sparse;
  if (!n_sparse) return JG_OK;
  if (o.keep) HIPCHK(hipStreamSynchronize(e->stream));
  InStep in_step(nd.in_step);
  int rc = JG_OK;
  // (a hosted step: the kernels of its catch-up pass assume the own slot its first pass assumed - its opens come behind them)
  struct OwnSlot {
    int& now;
    const int after;
    OwnSlot(int& v, int during) : now(v), after(v) { now = during; }
    ~OwnSlot() { now = after; }
  } own_slot(e->uniform_self, o.keep && o.hs.on ? o.hs.self0 : e->uniform_self);
  const uint32_t seq_end = e->seq;
  e->seq = pd.seq_general;
  const size_t recs_before = e->recs.size();
  if ((rc = node_general(e, pd.rows, pd.n, pd.nb, n_sparse, pd.now_ms))) return rc;
  // the general path's record belongs BEFORE the dense halves' fsm record (steps in order)
  if (e->recs.size() == recs_before + 1) {
    size_t at = recs_before;
    while (at > 0 && e->recs[at - 1].seq > pd.seq_general) at--;
    std::rotate(e->recs.begin() + at, e->recs.begin() + recs_before, e->recs.end());
  }
  uint64_t bytes_down = 0;
  e->seq = pd.seq_general;  // (the halves number themselves from here exactly as in the first pass)
  if ((rc = node_dense_halves(e, pd.now_ms, pd.flags, pd.col_mask, 2u, &bytes_down))) return rc;
  if (o.keep) {  // the step's fsm rows once more, from the deltas the catch-up pass completed
    if ((rc = node_keep_tail(e, pd.flags))) return rc;
    if (o.poll.want) {  // ... and its poll: the first pass saw the count and peeked - the same request, ungated, on the settled state
      o.poll.redone = true;
      if ((rc = node_poll_tail(e, o, nullptr))) return rc;
    }
    if (o.aw.on) {  // ... and its completion request: the gated chain appended nothing, removed nothing and left the head alone
      o.aw.redone = true;
      if ((rc = node_await_tail(e, o, nullptr))) return rc;
    }
    if (o.lk.on) {  // ... and its point query: the gated launch wrote no row
      o.lk.redone = true;
      if ((rc = node_lookup_tail(e, o, nullptr))) return rc;
    }
    if (o.hs.on) {  // ... and, last, its hosting request: the gated passes wrote nothing
      o.hs.redone = true;
      if ((rc = node_hosting_tail(e, o, nullptr))) return rc;
    }
    HIPCHK(hipEventRecord(o.ev_out, nd.down));
  }
  for (StepRec& rec : e->recs)
    if (!o.keep && rec.seq == pd.fsm_rec_seq && rec.fsm_per_row == JGN_FSM_ROWS && rec.msg_per_row == 0 && (rc = node_fsm_record(e, rec, pd.flags))) return rc;
  e->seq = seq_end;
  HIPCHK(hipStreamSynchronize(e->stream));
  return JG_OK;
}

// JG_NODE_KEEP: the fsm_tx rows of the step's dense halves, compacted and on their way home behind the step's own kernels -
// what jg_drain_applies does for a step record (scan of the tile sums, gather, one copy), enqueued HERE, the copy sized
// from the kept step finished last (the row count of a tick wobbles by a few percent at most; whatever is missing is
// fetched when the outbox is viewed) - then the status block as the step leaves it.  No drain is issued by the host.
int node_keep_tail(jg_engine* e, uint32_t flags) {
  jg_engine::NodeStep& nd = e->node;
  jg_engine::NodeOut& o = nd.cur();
  const uint32_t G = e->cfg.n_groups;
  const uint32_t n_tiles = (G + JG_SCAN_TILE - 1) / JG_SCAN_TILE;
  const size_t cap = (size_t)G * JGN_FSM_ROWS;
  if (!o.d_fsm) {
    Arena& ar = e->arenas[o.arena];
    HIPCHK(ar.alloc((size_t)G * 4, (void**)&o.d_fsm_cnt));
    HIPCHK(ar.alloc(cap * sizeof(jg_fsm_row), (void**)&o.d_fsm));
    HIPCHK(ar.alloc((size_t)n_tiles * 8, (void**)&o.d_bsum));
    HIPCHK(ar.alloc(cap * sizeof(jg_fsm_row), (void**)&o.d_stage));
  }
  hipLaunchKernelGGL(k_node_fsm_build, dim3(n_tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, nd.cols, o.d_fsm, o.d_fsm_cnt, o.d_bsum,
                     (flags & JG_NODE_FSM_FUSED) ? 1u : 0u);
  o.h_job[0] = JgScanJob{o.d_bsum, n_tiles, 0};
  hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(JG_BLOCK), 0, e->stream, (const JgScanJob*)o.h_job, o.h_total);
  hipLaunchKernelGGL(k_scan_gather<jg_fsm_row>, dim3(n_tiles), dim3(JG_BLOCK), 0, e->stream, o.d_fsm_cnt, G, o.d_bsum, (uint32_t)JGN_FSM_ROWS, o.d_fsm,
                     o.d_stage);
  HIPCHK(hipGetLastError());
  e->n_launch += 3;
  const size_t last = nd.fsm_guess_known ? nd.fsm_guess : (size_t)G;  // (no kept step finished yet: a row per partition)
  const size_t guess = std::min(cap, last + last / 32 + 4096);  // (3 % of room: every byte crosses the bus)
  o.l_fsm.n = 0;
  // (the status block is the step's own snapshot: taken on the step's stream, before a newer step's kernels touch it)
  HIPCHK(hipMemcpyAsync(o.h_status, e->d_status, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipEventRecord(o.ev_kernels, e->stream));
  HIPCHK(hipStreamWaitEvent(nd.down, o.ev_kernels, 0));
  if (guess) {
    HIPCHK(o.l_fsm.reserve(guess));
    HIPCHK(hipMemcpyAsync(o.l_fsm.p, o.d_stage, guess * sizeof(jg_fsm_row), hipMemcpyDeviceToHost, nd.down));
  }
  o.fsm_copied = guess;
  return JG_OK;
}

// JG_NODE_KEEP: the outbox of kept step `o` is being viewed - wait for ITS outputs (not for a newer step's), surface what
// its status block says, collect what only a step outside the steady state leaves behind (general-path records,
// exceptional rows, faults: the synchronous drain, over this step's queues and arena), and make its fsm rows the ones
// the next drain of that queue delivers.
int node_keep_finish(jg_engine* e, jg_engine::NodeOut& o) {
  jg_engine::NodeStep& nd = e->node;
  HIPCHK(hipSetDevice(e->device));
  int rc = JG_OK;
  if (&o == &nd.cur() && (rc = node_settle(e))) return rc;  // (the newest step: nobody has looked at its row count yet)
  HIPCHK(hipEventSynchronize(o.ev_out));
  const uint32_t* st = o.h_status;
  if ((rc = status_check(e, st))) return rc;
  if (e->flag_check_pending && o.irr_gen == e->irr_gen) {  // (as a pipelined drain's snapshot: no step since could have left an irregular chain)
    e->maybe_irregular = st[1] != 0;
    e->flag_check_pending = false;
  }
  if (st[5]) e->maybe_irregular = true;
  if (!e->slow_scheduled_ever && st[2]) return fail(JG_EDEVICE, "internal: irregular chain reached the fast-only dense path");
  const uint32_t nf = st[o.set ? 6 : 3], nx = st[o.set ? 7 : 4];
  if ((rc = node_keep_handover(e))) return rc;  // (the step before's rows, if nobody drained them: they come first)
  // (records of THIS step and of what came before it: a newer kept step that somebody settled meanwhile - a read of the
  // engine - keeps its own for its own view)
  size_t nrec = 0;
  while (nrec < e->recs.size() && e->recs[nrec].seq <= o.seq_hi) nrec++;
  if (nrec || nf || nx) {
    // outside the steady state: everything in flight first (the newer step's kernels too), then the synchronous drain
    HIPCHK(hipStreamSynchronize(e->stream));
    jg_engine::DrainBatch b;
    b.set = o.set;
    b.seq_hi = o.seq_hi;
    b.nf = nf, b.nx = nx;
    std::vector<StepRec> mine(e->recs.begin(), e->recs.begin() + nrec);
    e->recs.erase(e->recs.begin(), e->recs.begin() + nrec);
    if ((rc = drain_scan(e, mine, e->stream))) return rc;
    if (nrec) HIPCHK(hipStreamSynchronize(e->stream));
    if ((rc = drain_gather(e, b, mine, e->stream))) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    if ((rc = drain_finish(e, b, mine, nullptr))) return rc;  // (the arena: below, once everything in it has been read)
    e->fault_floor[b.set] = b.seq_hi;
  }
  const size_t total = (size_t)*o.h_total;
  if (total > o.fsm_copied) {  // (the copy behind the step was sized from the step before: the rest now)
    o.l_fsm.n = o.fsm_copied;
    HIPCHK(o.l_fsm.reserve(total));
    HIPCHK(hipMemcpyAsync(o.l_fsm.p + o.fsm_copied, o.d_stage + o.fsm_copied, (total - o.fsm_copied) * sizeof(jg_fsm_row), hipMemcpyDeviceToHost,
                          e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  o.l_fsm.n = total, o.fsm_landed = total != 0;
  if (e->track_segs) seg_add(e->seg_f, o.seq_hi, total);
  nd.fsm_guess = total, nd.fsm_guess_known = true;
  if ((rc = node_poll_finish(e, o))) return rc;  // (the rows its own copy did not bring: out of the arena, before it starts over)
  if ((rc = node_await_finish(e, o))) return rc;
  if ((rc = node_lookup_finish(e, o))) return rc;
  if ((rc = node_hosting_finish(e, o))) return rc;
  // everything the step allocated has been read - d_stage just above was the last: its arena starts over, here and nowhere
  // else (records, if it had any, were drained above)
  e->arenas[o.arena].reset();
  o.d_fsm_cnt = nullptr, o.d_fsm = o.d_stage = nullptr, o.d_bsum = nullptr;
  o.out = false;
  nd.kept_n--;
  return JG_OK;
}
}  // namespace

int jg_step_node(jg_engine* e, uint64_t now_ms, uint32_t flags) {
  if (!e) return fail(JG_EINVAL, "null argument");
  if (!(flags & (JG_NODE_LEADER_HALF | JG_NODE_FOLLOWER_HALF)) || (flags & ~127u))
    return fail(JG_EINVAL, "jg_step_node: flags = JG_NODE_LEADER_HALF and / or JG_NODE_FOLLOWER_HALF [| JG_NODE_TICK] [| JG_NODE_ASYNC] [| JG_NODE_COMMON_AE] [| JG_NODE_FSM_FUSED] [| JG_NODE_KEEP]");
  if (e->router && (flags & (JG_NODE_COMMON_AE | JG_NODE_KEEP))) return fail(JG_EINVAL, "jg_step_node: JG_NODE_COMMON_AE and JG_NODE_KEEP are per shard (jg_get_shard)");
  if (e->router) return router_step_node(e, now_ms, flags);
  if (e->inflight.phase) return fail(JG_EINVAL, "a drain is in transfer: jg_drain_wait first");
  return node_step(e, now_ms, flags, nullptr);
}

int jg_node_inbox_columns(jg_engine* e, uint32_t slot, uint64_t** answer, uint64_t** hb_commit) {
  if (!e || !answer) return fail(JG_EINVAL, "null argument");
  if (e->router) return fail(JG_EINVAL, "jg_node_inbox_columns: the columns are per shard: call this on a shard handle (jg_get_shard)");
  if (slot >= e->cfg.n_replicas) return fail(JG_EINVAL, "slot out of range");
  if (e->uniform_self >= 0 && (uint32_t)e->uniform_self == slot)
    return fail(JG_EINVAL, "jg_node_inbox_columns: the own slot's word carries the append count");
  HIPCHK(hipSetDevice(e->device));
  int rc = node_ensure(e);
  if (rc) return rc;
  jg_engine::NodeStep& nd = e->node;
  const size_t G = e->cfg.n_groups;
  if (nd.cols_in_flight) {  // the previous step's uploads out of these buffers (a step without rows never synchronises)
    HIPCHK(hipEventSynchronize(nd.ev_cols));
    nd.cols_in_flight = false;
  }
  *answer = nd.h_in_answers + (size_t)slot * G;
  nd.col_mask |= 1u << slot;
  if (hb_commit) {
    *hb_commit = nd.h_in_hbc + (size_t)slot * G;
    nd.col_hbc_mask |= 1u << slot;
  } else {
    nd.col_hbc_mask &= ~(1u << slot);
  }
  return JG_OK;
}

int jg_node_outbox_view(jg_engine* e, jg_node_outbox* out) {
  if (!e || !out) return fail(JG_EINVAL, "null argument");
  if (e->router) return router_node_outbox(e, out);
  jg_engine::NodeStep& nd = e->node;
  if (!nd.ready || !(nd.sets[0].last_flags | nd.sets[1].last_flags)) return fail(JG_EINVAL, "no jg_step_node yet");
  // JG_NODE_KEEP: the OLDEST step whose outbox has not been viewed; none outstanding: the one viewed last, again
  jg_engine::NodeOut& o = nd.to_view();
  int rc = JG_OK;
  if (o.out) {
    if ((rc = node_keep_finish(e, o))) return rc;  // (waits for THIS step's outputs only)
  } else if (!nd.kept_n) {
    if ((rc = sync_and_check(e))) return rc;  // (the columns have landed; device-side error flags surface here)
  }
  *out = o.last;
  if ((o.last_flags & JG_NODE_LEADER_HALF) && (o.last_flags & JG_NODE_TICK)) {
    out->beat = o.h_beat, out->ae = o.h_ae;
    if (o.last_flags & JG_NODE_COMMON_AE) {
      out->aec = o.h_aec, out->ae = nullptr;
      if (o.h_nsparse[2]) {  // some partition's words differ by addressee: the rows are wanted after all
        if (!o.ae_rows_landed) {
          HIPCHK(hipSetDevice(e->device));
          // (a kept step: its own copy of the rows - a newer step has written the other set's since)
          if ((rc = node_fetch_ae_rows(e, o, e->stream, &o.last.bytes_d2h))) return rc;
          HIPCHK(hipStreamSynchronize(e->stream));
          out->bytes_d2h = o.last.bytes_d2h;
          o.ae_rows_landed = true;
        }
        out->ae = o.h_ae;
      }
    }
  }
  if (o.last_flags & JG_NODE_FOLLOWER_HALF) out->answer = o.h_answer, out->hb_commit = o.h_hbc;
  return JG_OK;
}
