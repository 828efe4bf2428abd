// jg_api_await.h - jg_engine_await_open / jg_engine_await_blocks / jg_engine_await_cancel / jg_engine_watch_completions: the
// completion feed (jg_await.h).  Calls that read, under the rules of jg_api_manage.h: refused while kept node steps are
// outstanding, JG_NODE_ASYNC steps settled, the rows' landing area carved from the engine's staging, a multi-device handle
// served shard by shard.  A watch queues its passes back to back and synchronises once; a registration is one host-to-device copy
// behind the table's end.  The feed walks a table, not a slot range, so it keeps a chain of its own (await_shard) beside
// the other feeds' one host path (jg_api_poll.h), in the same three pieces: await_plan hands out the geometry and the
// sections of one block, await_bind the arguments over whoever's block it is, await_queue the chain.  The synchronous watch
// is those pieces over the engine's staging with the host's n and cur; an AWAITED node step (jg_step_node_awaited, ABI v23:
// node_await_stage / node_await_tail / node_await_finish, called by jg_api_node.h) is the same pieces over a block of the
// kept-step set's arena with the table's head read on the device.  Part of josefine_gpu.hip's one translation unit.
#pragma once

namespace {

// offsets in AwaitTable::misc
constexpr size_t AWT_O_TOTAL = 0, AWT_O_SUM = 16, AWT_O_JOB = 64, AWT_O_HEAD = 128, AWT_O_MARKED = 144, AWT_MISC_BYTES = 160;
static_assert(AWT_O_SUM + JG_AWT_WORDS * 8 <= AWT_O_JOB && AWT_O_JOB + sizeof(JgScanJob) <= AWT_O_HEAD, "AwaitTable::misc");
static_assert(AWT_O_HEAD % 16 == 0 && AWT_O_HEAD + sizeof(JgAwaitHead) <= AWT_O_MARKED, "AwaitTable::misc: the head");
static_assert(AWT_O_MARKED + 8 <= AWT_MISC_BYTES, "AwaitTable::misc: the marked count");
// (a waiter's index, and the tile count, are 32-bit in the kernels)
constexpr size_t AWT_MAX_CAPACITY = 0xFFFF0000ull;

// one single-device engine's table (re)sized: refused while waiters are outstanding; 0 frees it
int await_open_shard(jg_engine* e, size_t capacity) {
  jg_engine::AwaitTable& t = e->await;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));  // (nothing queued reads the buffers that go)
  t.release();
  if (!capacity) return JG_OK;
  const size_t tiles = (capacity + JG_AWT_TILE - 1) / JG_AWT_TILE;
  int rc = JG_OK;
  auto get = [&](auto** p, size_t bytes) {
    if (!rc && hipMalloc((void**)p, std::max<size_t>(bytes, 16)) != hipSuccess) rc = fail(JG_ENOMEM, "jg_engine_await_open: out of device memory");
  };
  get(&t.buf[0], capacity * sizeof(jg_await_row));
  get(&t.buf[1], capacity * sizeof(jg_await_row));
  get(&t.verdict, capacity);
  get(&t.bsum, tiles * 8);
  get(&t.part, (size_t)JG_AWT_PARTS * JG_AWT_WORDS * 8);
  get(&t.mpart, (size_t)JG_AWT_PARTS * 8);  // (the mark pass's own: the count pass of the same chain overwrites `part`)
  get(&t.misc, AWT_MISC_BYTES);
  if (rc) {
    t.release();
    return rc;
  }
  t.cap = capacity;
  return JG_OK;
}

// rows (shard-local groups, checked) behind the table's end of one single-device engine; the capacity was checked
int await_append_shard(jg_engine* e, const jg_await_row* rows, size_t n) {
  if (!n) return JG_OK;
  jg_engine::AwaitTable& t = e->await;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipMemcpyAsync((char*)t.buf[t.cur] + t.n * sizeof(jg_await_row), rows, n * sizeof(jg_await_row), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  t.n += n;
  return JG_OK;
}

// One watch's chain of kernels over ONE block of scratch (the rows' landing area; an awaited step's staged rows and header
// block too): the table's own buffers, verdict bytes, tile counts and partial records serve both.  `kept`: the chain of an
// awaited node step - the head is the device's, n is the host's bound on it.  A synchronous cancel is the same plan with
// nothing to deliver and its keys in the block: the mark pass alone.
struct AwaitPlan {
  bool kept = false;
  uint32_t n = 0, tiles = 0, parts = 0;  // the waiters the passes are launched for
  size_t m = 0, wcap = 0;                // staged rows (kept); rows the landing area holds
  size_t ck = 0;                         // the cancel's keys (kept: staged behind the rows; synchronous: a cancel's plan alone)
  Carve c;
  size_t o_out = 0, o_rows = 0, o_hdr = 0, o_keys = 0;
  JgAwaitArgs a{};
};

void await_plan(AwaitPlan& P, bool kept, size_t n, size_t m, size_t cap, size_t ck = 0) {
  P.kept = kept, P.n = (uint32_t)n, P.m = m, P.ck = ck;
  P.tiles = std::max<uint32_t>((P.n + JG_AWT_TILE - 1) / JG_AWT_TILE, kept ? 1u : 0u);  // (an awaited step's header wants its total: one tile at least)
  P.parts = std::min<uint32_t>(P.tiles, JG_AWT_PARTS);
  P.wcap = std::min<size_t>(cap, n);
  P.o_out = P.c.sect(P.wcap * sizeof(jg_done_row));
  if (kept) P.o_rows = P.c.sect(m * sizeof(jg_await_row)), P.o_hdr = P.c.sect(JG_AH_WORDS * 8);
  if (kept || ck) P.o_keys = P.c.sect(ck * 8);
}

// the arguments of every pass over block B, one record (JgAwaitArgs): what both chains read, then what each reads alone;
// `gate`: null, or the device word that makes an awaited step's chain leave everything alone (jg_await.h)
void await_bind(jg_engine* e, AwaitPlan& P, char* B, bool peek, bool stats, uint64_t now_ms, uint32_t add, const uint32_t* gate,
                uint64_t cmask = 0) {
  jg_engine::AwaitTable& t = e->await;
  JgAwaitArgs& a = P.a;
  a.peek = peek ? 1u : 0u, a.tiles = P.tiles, a.parts = P.parts, a.n_keys = (uint32_t)P.ck;
  a.now = now_ms, a.cap = P.wcap, a.mask = cmask;
  a.buf[0] = t.buf[0], a.buf[1] = t.buf[1], a.verdict = t.verdict, a.bsum = t.bsum, a.part = t.part;
  a.total = (const uint64_t*)(t.misc + AWT_O_TOTAL), a.out = (uint4*)(B + P.o_out);
  a.keys = (const uint64_t*)(B + P.o_keys), a.mpart = t.mpart;
  if (!P.kept) {  // the table's view is the host's
    a.n = P.n, a.cur = (uint32_t)t.cur, a.add = add;
    a.sum = (uint64_t*)(t.misc + AWT_O_SUM), a.marked = (uint64_t*)(t.misc + AWT_O_MARKED);
  } else {  // ... the head's
    a.m = (uint32_t)P.m, a.room = (uint32_t)t.cap, a.stats = stats ? 1u : 0u;
    a.head = (JgAwaitHead*)(t.misc + AWT_O_HEAD), a.gate = gate;
    a.rows = (const uint4*)(B + P.o_rows), a.hdr = (uint64_t*)(B + P.o_hdr);
  }
}

// the whole chain on the engine's stream (`job`: where the device reads the scan job): [the append, the mark pass,] the
// count pass, the scan, the stats sum if wanted, the write pass - queued unseen: with nothing done every workgroup returns after its first
// loads - [and the header kernel, which folds the stats itself]
int await_queue(jg_engine* e, const AwaitPlan& P, const JgScanJob* job, bool stats) {
  jg_engine::AwaitTable& t = e->await;
  const dim3 block(JG_BLOCK);
  uint64_t* const total = (uint64_t*)(t.misc + AWT_O_TOTAL);
  if (!P.kept) {
    hipLaunchKernelGGL(k_await_count, dim3(P.parts), block, 0, e->stream, e->dev, P.a);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), block, 0, e->stream, job, total);
    e->n_launch += 2;
    if (stats) {
      hipLaunchKernelGGL(k_await_stats_sum, dim3(1), block, 0, e->stream, P.a);
      e->n_launch++;
    }
    if (P.wcap) {
      hipLaunchKernelGGL(k_await_write, dim3(P.tiles), block, 0, e->stream, e->dev, P.a);
      e->n_launch++;
    }
  } else {
    if (P.m) {
      hipLaunchKernelGGL(k_await_append, dim3((uint32_t)((P.m * 3 + JG_BLOCK - 1) / JG_BLOCK)), block, 0, e->stream, P.a);
      e->n_launch++;
    }
    if (P.ck) {  // (behind the append: the step's own rows can be withdrawn by it)
      hipLaunchKernelGGL(k_await_mark_kept, dim3(P.parts), block, 0, e->stream, P.a);
      e->n_launch++;
    }
    hipLaunchKernelGGL(k_await_count_kept, dim3(P.parts), block, 0, e->stream, e->dev, P.a);
    hipLaunchKernelGGL(k_scan_block_sums, dim3(1), block, 0, e->stream, job, total);
    if (P.wcap) {
      hipLaunchKernelGGL(k_await_write_kept, dim3(P.tiles), block, 0, e->stream, e->dev, P.a);
      e->n_launch++;
    }
    hipLaunchKernelGGL(k_await_header, dim3(1), block, 0, e->stream, P.a);
    e->n_launch += 3;
  }
  HIPCHK(hipGetLastError());
  return JG_OK;
}

// one single-device engine's part of a completion watch: the first `cap` done waiters (groups + add) into host `out`,
// removed unless peeking; *total the done waiters; w (if not null) [JG_AWT_WORDS] the stats before the delivery
int await_shard(jg_engine* e, uint32_t flags, uint64_t now_ms, uint32_t add, jg_done_row* out, size_t cap, size_t* total, uint64_t* w) {
  *total = 0;
  if (w) std::memset(w, 0, JG_AWT_WORDS * 8);
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = node_settle(e);
    if (rc) return rc;
  }
  jg_engine::AwaitTable& t = e->await;
  if (!t.n) return JG_OK;
  const bool peek = (flags & JG_WATCH_PEEK) != 0;
  AwaitPlan P;
  await_plan(P, false, t.n, 0, cap);
  char* B = nullptr;
  if (const int rc = P.c.on_staging(e, B)) return rc;
  await_bind(e, P, B, peek, w != nullptr, now_ms, add, nullptr);
  const JgScanJob job{t.bsum, P.tiles, 0};
  HIPCHK(hipMemcpyAsync(t.misc + AWT_O_JOB, &job, sizeof job, hipMemcpyHostToDevice, e->stream));
  if (const int rc = await_queue(e, P, (const JgScanJob*)(t.misc + AWT_O_JOB), w != nullptr)) return rc;
  uint64_t tot = 0;
  HIPCHK(hipMemcpyAsync(&tot, t.misc + AWT_O_TOTAL, 8, hipMemcpyDeviceToHost, e->stream));
  if (w) HIPCHK(hipMemcpyAsync(w, P.a.sum, JG_AWT_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *total = (size_t)tot;
  const size_t k = std::min<size_t>(P.wcap, tot);
  if (k) HIPCHK(hipMemcpy(out, P.a.out, k * sizeof(jg_done_row), hipMemcpyDeviceToHost));
  if (k && !peek) t.cur ^= 1, t.n -= k;  // the survivors are in the other buffer
  return JG_OK;
}

// one single-device engine's part of a cancel: the mark pass over its table and the reduce, planned and bound as a watch
// is, the keys (sorted, distinct, within mask: await_keys_check) staged into the engine's staging; *marked the waiters
// newly marked.  The caller has settled the engine's JG_NODE_ASYNC step
int await_cancel_shard(jg_engine* e, const std::vector<uint64_t>& keys, uint64_t mask, size_t* marked) {
  *marked = 0;
  HIPCHK(hipSetDevice(e->device));
  jg_engine::AwaitTable& t = e->await;
  if (!t.n) return JG_OK;
  AwaitPlan P;
  await_plan(P, false, t.n, 0, 0, keys.size());
  char* B = nullptr;
  if (const int rc = P.c.on_staging(e, B)) return rc;
  await_bind(e, P, B, false, false, 0, 0, nullptr, mask);
  HIPCHK(hipMemcpyAsync(B + P.o_keys, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_await_mark, dim3(P.parts), dim3(JG_BLOCK), 0, e->stream, P.a);
  hipLaunchKernelGGL(k_await_mark_sum, dim3(1), dim3(JG_BLOCK), 0, e->stream, P.a);
  e->n_launch += 2;
  HIPCHK(hipGetLastError());
  uint64_t got = 0;
  HIPCHK(hipMemcpyAsync(&got, P.a.marked, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *marked = (size_t)got;
  return JG_OK;
}

// the rules of jg_engine_await_cancel for a key set; `out`: the keys copied, sorted, duplicates removed
int await_keys_check(const uint64_t* keys, size_t n, uint64_t mask, const char* who, std::vector<uint64_t>& out) {
  if (n && !keys) return fail(JG_EINVAL, "null argument");
  if (n > JG_AWAIT_CANCEL_MAX) return fail(JG_EINVAL, std::string(who) + ": more than JG_AWAIT_CANCEL_MAX keys");
  for (size_t i = 0; i < n; i++)
    if (keys[i] & ~mask) return fail(JG_EINVAL, std::string(who) + ": a key has a bit outside the mask (it could never match)");
  out.assign(keys, keys + n);
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
  return JG_OK;
}

// the rules of jg_engine_await_blocks for rows that are about to be registered on a single-device engine
int await_rows_check(const jg_engine* e, const jg_await_row* rows, size_t n, const char* who) {
  auto refuse = [&](const char* what) { return fail(JG_EINVAL, std::string(who) + ": " + what); };
  for (size_t i = 0; i < n; i++) {
    const jg_await_row& r = rows[i];
    if (r.group >= e->cfg.n_groups) return refuse("group out of range");
    if (r.flags || r.reserved) return refuse("flags and reserved must be 0");
    if (!r.block_id) return refuse("block id 0 is never applied");
  }
  return JG_OK;
}

// ---- completions behind a kept node step (jg_step_node_awaited) ----------------------------------------------------------
// the set's pinned words: the scan job and the head the device reads, then where the header block lands
enum { NODE_AWAIT_JOB = 0, NODE_AWAIT_HEAD = 2, NODE_AWAIT_HDR = 4, NODE_AWAIT_PINNED_WORDS = NODE_AWAIT_HDR + JG_AH_WORDS };
static_assert(sizeof(JgScanJob) <= 16, "the job fits in front of the head");

// the host's bound on the waiters outstanding: as of the newest viewed step or synchronous call, plus what the steps begun
// since register
size_t node_await_bound(const jg_engine* e) {
  size_t b = e->await.n;
  for (const jg_engine::NodeOut& o : e->node.sets)
    if (o.out && o.aw.on) b += o.aw.m;
  return b;
}

// the step's rows, and behind them its cancel keys, into the set's pinned memory (the set is the step's from here on;
// whatever read it last has been viewed)
int node_await_stage(jg_engine::NodeOut& o, const jg_await_row* rows, const uint64_t* keys) {
  const size_t bytes = o.aw.m * sizeof(jg_await_row), kbytes = o.aw.ck * 8;
  o.l_await_up.n = 0;
  if (!(bytes + kbytes)) return JG_OK;
  HIPCHK(o.l_await_up.reserve(bytes + kbytes));
  if (bytes) std::memcpy(o.l_await_up.p, rows, bytes);
  if (kbytes) std::memcpy(o.l_await_up.p + bytes, keys, kbytes);
  return JG_OK;
}

// The completion request of kept step `o`, queued behind the kernels of that step (and its poll) that are in the stream by
// now, and its trip home on the down stream: the header block as one copy, the done rows sized from the awaited step
// finished last (the rest is fetched when the step is viewed: node_await_finish).  The first pass sends the staged rows up,
// behind the step, and - if no awaited step is outstanding, so that the host's n and cur are the table's - writes the head
// from them, in the stream.  `gate`: as for node_poll_tail.  Synchronises nothing.
int node_await_tail(jg_engine* e, jg_engine::NodeOut& o, const uint32_t* gate) {
  jg_engine::NodeStep& nd = e->node;
  jg_engine::NodeAwait& aw = o.aw;
  jg_engine::AwaitTable& t = e->await;
  AwaitPlan P;
  await_plan(P, true, aw.bound, aw.m, aw.cap, aw.ck);
  if (!aw.scratch) HIPCHK(e->arenas[o.arena].alloc(P.c.at, (void**)&aw.scratch));  // (the pass behind the catch-up pass: the same block)
  if (!o.h_await) {
    HIPCHK(hipHostMalloc((void**)&o.h_await, NODE_AWAIT_PINNED_WORDS * 8, hipHostMallocDefault));
    std::memset(o.h_await, 0, NODE_AWAIT_PINNED_WORDS * 8);
  }
  char* const B = aw.scratch;
  await_bind(e, P, B, aw.peek, aw.stats, aw.now_ms, 0, gate, aw.cmask);
  if (!aw.redone) {
    if (aw.m) HIPCHK(hipMemcpyAsync(B + P.o_rows, o.l_await_up.p, aw.m * sizeof(jg_await_row), hipMemcpyHostToDevice, e->stream));
    if (aw.ck) HIPCHK(hipMemcpyAsync(B + P.o_keys, o.l_await_up.p + aw.m * sizeof(jg_await_row), aw.ck * 8, hipMemcpyHostToDevice, e->stream));
    const jg_engine::NodeOut& other = nd.sets[(&o - nd.sets) ^ 1];
    if (!(other.out && other.aw.on)) {  // (the step before, if it is outstanding and awaited, leaves the head behind its chain)
      JgAwaitHead* const h = (JgAwaitHead*)(o.h_await + NODE_AWAIT_HEAD);
      *h = JgAwaitHead{(uint32_t)t.n, (uint32_t)t.cur, {0u, 0u}};
      HIPCHK(hipMemcpyAsync(t.misc + AWT_O_HEAD, h, sizeof *h, hipMemcpyHostToDevice, e->stream));
    }
  }
  *(JgScanJob*)(o.h_await + NODE_AWAIT_JOB) = JgScanJob{t.bsum, P.tiles, 0};
  if (const int rc = await_queue(e, P, (const JgScanJob*)(o.h_await + NODE_AWAIT_JOB), aw.stats)) return rc;
  HIPCHK(hipEventRecord(o.ev_kernels, e->stream));
  HIPCHK(hipStreamWaitEvent(nd.down, o.ev_kernels, 0));
  HIPCHK(hipMemcpyAsync(o.h_await + NODE_AWAIT_HDR, P.a.hdr, JG_AH_WORDS * 8, hipMemcpyDeviceToHost, nd.down));
  if (!aw.redone) {  // (the pass behind the catch-up pass lands where the first one did: its copy may still be in flight)
    const size_t last = nd.await_guess_known ? nd.await_guess : P.wcap;  // (no awaited step finished yet: min(cap, bound))
    aw.copied = std::min(P.wcap, last + last / 32 + 4096);               // (the margin of the fsm rows: node_keep_tail)
  }
  if (const size_t bytes = aw.copied * sizeof(jg_done_row)) {
    o.l_await.n = 0;
    HIPCHK(o.l_await.reserve(bytes));
    HIPCHK(hipMemcpyAsync(o.l_await.p, P.a.out, bytes, hipMemcpyDeviceToHost, nd.down));
  }
  return JG_OK;
}

// Kept step `o` is being viewed and its outputs have landed: the header block says what was delivered - the rows the step's
// own copy did not bring are fetched now - and what the table's head is behind the step: the host's n, cur and bound follow
// it.  The answer is what jg_node_await_view hands out from here on.  Before the set's arena starts over.
int node_await_finish(jg_engine* e, jg_engine::NodeOut& o) {
  jg_engine::NodeStep& nd = e->node;
  jg_engine::NodeAwait& aw = o.aw;
  jg_engine::AwaitTable& t = e->await;
  jg_node_await& v = o.await_view;
  v = jg_node_await{};
  if (!aw.on) return JG_OK;
  const uint64_t* const h = o.h_await + NODE_AWAIT_HDR;
  if (h[JG_AH_GATE]) return fail(JG_EDEVICE, "internal: an awaited step's chain was gated and not queued again");
  AwaitPlan P;
  await_plan(P, true, aw.bound, aw.m, aw.cap, aw.ck);
  const size_t given = (size_t)h[JG_AH_GIVEN];
  if (given > P.wcap || h[JG_AH_N] > t.cap) return fail(JG_EDEVICE, "internal: an awaited step's header block is out of range");
  if (given > aw.copied) {
    o.l_await.n = aw.copied * sizeof(jg_done_row);  // (what has landed moves along if the buffer grows)
    HIPCHK(o.l_await.reserve(given * sizeof(jg_done_row)));
    HIPCHK(hipMemcpyAsync(o.l_await.p + aw.copied * sizeof(jg_done_row), aw.scratch + P.o_out + aw.copied * sizeof(jg_done_row),
                          (given - aw.copied) * sizeof(jg_done_row), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  nd.await_guess = (size_t)h[JG_AH_TOTAL], nd.await_guess_known = true;
  t.n = (size_t)h[JG_AH_N], t.cur = (int)(h[JG_AH_CUR] & 1u);
  v.attached = 1u, v.state = aw.redone ? (uint32_t)JG_NODE_POLL_REDONE : 0u;
  v.rows = given ? (const jg_done_row*)o.l_await.p : nullptr;
  v.rows_n = given, v.total = (size_t)h[JG_AH_TOTAL], v.marked = (size_t)h[JG_AH_MARKED];
  if (aw.stats) {  // (jg_await_stats is the stat words in order, then left: jg_await.h)
    std::memcpy(&v.stats, h + JG_AH_STATS, JG_AWT_WORDS * 8);
    v.stats.left = h[JG_AH_LEFT];
  }
  aw.scratch = nullptr;  // (the arena's: gone with it)
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_engine_await_open(jg_engine* e, size_t capacity) {
  if (!e) return fail(JG_EINVAL, "null argument");
  if (capacity > AWT_MAX_CAPACITY) return fail(JG_EINVAL, "jg_engine_await_open: capacity too large");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  for (size_t d = 0; d < shard_count(e); d++)
    if (shard_at(e, d)->await.n) return fail(JG_EINVAL, "jg_engine_await_open: waiters are outstanding");
  return each_shard(e, [&](size_t d) -> int { return await_open_shard(shard_at(e, d), capacity); });
}

int jg_engine_await_blocks(jg_engine* e, const jg_await_row* rows, size_t n) {
  if (!e || (n && !rows)) return fail(JG_EINVAL, "null argument");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  if (!shard_at(e, 0)->await.cap) return fail(JG_EINVAL, "jg_engine_await_blocks: no open table (jg_engine_await_open)");
  if (const int rc = await_rows_check(e, rows, n, "jg_engine_await_blocks")) return rc;
  if (!e->router) {
    if (e->await.n + n > e->await.cap) return fail(JG_ECAPACITY, "jg_engine_await_blocks: the table is full");
    HIPCHK(hipSetDevice(e->device));
    if (const int rc = node_settle(e)) return rc;
    return await_append_shard(e, rows, n);
  }
  // a sharded handle: the rows bucketed by owner shard, stably, their groups rebased; every shard's room checked first
  const size_t D = shard_count(e);
  const std::vector<uint32_t>& lo = e->router->lo;
  std::vector<std::vector<jg_await_row>> part(D);
  for (size_t i = 0; i < n; i++) {
    const size_t d = (size_t)(std::upper_bound(lo.begin(), lo.end(), rows[i].group) - lo.begin()) - 1;
    jg_await_row r = rows[i];
    r.group -= lo[d];
    part[d].push_back(r);
  }
  for (size_t d = 0; d < D; d++) {
    const jg_engine::AwaitTable& t = shard_at(e, d)->await;
    if (t.n + part[d].size() > t.cap) return fail(JG_ECAPACITY, "jg_engine_await_blocks: a shard's table is full");
  }
  return each_shard(e, [&](size_t d) -> int {
    jg_engine* s = shard_at(e, d);
    HIPCHK(hipSetDevice(s->device));
    if (const int rc = node_settle(s)) return rc;
    return await_append_shard(s, part[d].data(), part[d].size());
  });
}

int jg_engine_await_cancel(jg_engine* e, const uint64_t* keys, size_t n_keys, uint64_t mask, size_t* marked) {
  if (!e || !marked) return fail(JG_EINVAL, "null argument");
  std::vector<uint64_t> sorted;
  if (const int rc = await_keys_check(keys, n_keys, mask, "jg_engine_await_cancel", sorted)) return rc;
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  {  // JG_NODE_ASYNC steps are settled first, whatever the call then finds to do
    const int rc = each_shard(e, [&](size_t d) -> int {
      jg_engine* s = shard_at(e, d);
      HIPCHK(hipSetDevice(s->device));
      return node_settle(s);
    });
    if (rc) return rc;
  }
  const size_t D = shard_count(e);
  std::vector<size_t> got(D, 0);
  if (!sorted.empty() && shard_at(e, 0)->await.cap) {
    const int rc = each_shard(e, [&](size_t d) -> int { return await_cancel_shard(shard_at(e, d), sorted, mask, &got[d]); });
    if (rc) return rc;
  }
  size_t sum = 0;
  for (size_t d = 0; d < D; d++) sum += got[d];
  *marked = sum;
  return JG_OK;
}

int jg_engine_watch_completions(jg_engine* e, uint32_t flags, uint64_t now_ms, jg_done_row* out, size_t cap, size_t* total,
                                jg_await_stats* stats) {
  if (!e || !total || (cap && !out)) return fail(JG_EINVAL, "null argument");
  if (flags & ~(uint32_t)JG_WATCH_PEEK) return fail(JG_EINVAL, "jg_engine_watch_completions: unknown flag");
  if (now_ms == UINT64_MAX) return fail(JG_EINVAL, "jg_engine_watch_completions: now_ms out of range");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  uint64_t* sw = (uint64_t*)stats;  // (jg_await_stats is the stat words in order, then left: jg_await.h)
  const size_t D = shard_count(e);
  auto left = [&] {
    uint64_t t = 0;
    for (size_t d = 0; d < D; d++) t += shard_at(e, d)->await.n;
    return t;
  };
  if (!e->router) {  // (straight into the caller's array; the stats only once the call has succeeded)
    uint64_t w[JG_AWT_WORDS];
    size_t tot = 0;
    const int rc = await_shard(e, flags, now_ms, 0, out, cap, &tot, sw ? w : nullptr);
    if (rc) return rc;
    *total = tot;
    if (sw) std::memcpy(sw, w, sizeof w), sw[JG_AWT_WORDS] = left();
    return JG_OK;
  }
  // a sharded handle: every shard is sized first (a peek that delivers nothing; the stats are the shards' sums from that
  // pass), then each shard delivers - and removes - what is left of cap behind the shards before it; a shard behind the
  // point where cap ran out is not called again
  std::vector<size_t> tot(D, 0), at(D + 1, 0);
  std::vector<uint64_t> w(D * JG_AWT_WORDS, 0);
  int rc = each_shard(e, [&](size_t d) -> int {
    return await_shard(shard_at(e, d), flags | JG_WATCH_PEEK, now_ms, 0, nullptr, 0, &tot[d], sw ? w.data() + d * JG_AWT_WORDS : nullptr);
  });
  if (rc) return rc;
  for (size_t d = 0; d < D; d++) at[d + 1] = at[d] + tot[d];
  if (cap && at[D]) {
    rc = each_shard(e, [&](size_t d) -> int {
      if (!tot[d] || at[d] >= cap) return JG_OK;
      size_t again = 0;
      return await_shard(shard_at(e, d), flags, now_ms, e->router->lo[d], out + at[d], cap - at[d], &again, nullptr);
    });
    if (rc) return rc;
  }
  *total = at[D];
  if (sw) {
    std::memset(sw, 0, JG_AWT_WORDS * 8);
    for (size_t d = 0; d < D; d++) merge_words(sw, w.data() + d * JG_AWT_WORDS, JG_AWT_WORDS, summed);
    sw[JG_AWT_WORDS] = left();
  }
  return JG_OK;
}

}  // extern "C"
