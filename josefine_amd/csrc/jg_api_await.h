// jg_api_await.h - jg_engine_await_open / jg_engine_await_blocks / jg_engine_watch_completions: the completion feed
// (jg_await.h).  Calls that read, under the rules of jg_api_manage.h: refused while kept node steps are outstanding,
// JG_NODE_ASYNC steps settled, the rows' landing area carved from the engine's staging, a multi-device handle served shard
// by shard.  A watch queues its passes back to back and synchronises once; a registration is one host-to-device copy
// behind the table's end.  The feed walks a table, not a slot range, so it keeps a chain of its own (await_shard) beside
// the other feeds' one host path (jg_api_poll.h).  Part of josefine_gpu.hip's one translation unit.
#pragma once

namespace {

// offsets in AwaitTable::misc
constexpr size_t AWT_O_TOTAL = 0, AWT_O_SUM = 16, AWT_O_JOB = 64, AWT_MISC_BYTES = 128;
static_assert(AWT_O_SUM + JG_AWT_WORDS * 8 <= AWT_O_JOB && AWT_O_JOB + sizeof(JgScanJob) <= AWT_MISC_BYTES, "AwaitTable::misc");
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
  JgAwaitArgs a{};
  a.n = (uint32_t)t.n, a.add = add, a.peek = (flags & JG_WATCH_PEEK) ? 1u : 0u;
  a.tiles = (a.n + JG_AWT_TILE - 1) / JG_AWT_TILE;
  a.parts = std::min<uint32_t>(a.tiles, JG_AWT_PARTS);
  a.now = now_ms;
  const size_t wcap = std::min<size_t>(cap, t.n);
  Carve c;
  const size_t o_out = c.sect(wcap * sizeof(jg_done_row));
  char* B = nullptr;
  if (const int rc = c.on_staging(e, B)) return rc;
  a.cap = wcap;
  a.tab = t.buf[t.cur], a.dst = t.buf[t.cur ^ 1], a.verdict = t.verdict;
  a.bsum = t.bsum, a.part = t.part;
  a.sum = (uint64_t*)(t.misc + AWT_O_SUM), a.total = (const uint64_t*)(t.misc + AWT_O_TOTAL);
  a.out = (uint4*)(B + o_out);
  const JgScanJob job{a.bsum, a.tiles, 0};
  HIPCHK(hipMemcpyAsync(t.misc + AWT_O_JOB, &job, sizeof job, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_await_count, dim3(a.parts), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
  hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(JG_BLOCK), 0, e->stream, (const JgScanJob*)(t.misc + AWT_O_JOB), (uint64_t*)(t.misc + AWT_O_TOTAL));
  e->n_launch += 2;
  if (w) {
    hipLaunchKernelGGL(k_await_stats_sum, dim3(1), dim3(JG_BLOCK), 0, e->stream, a);
    e->n_launch++;
  }
  if (wcap) {  // (queued unseen: with nothing done every workgroup returns after its first load)
    hipLaunchKernelGGL(k_await_write, dim3(a.tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
    e->n_launch++;
  }
  HIPCHK(hipGetLastError());
  uint64_t tot = 0;
  HIPCHK(hipMemcpyAsync(&tot, t.misc + AWT_O_TOTAL, 8, hipMemcpyDeviceToHost, e->stream));
  if (w) HIPCHK(hipMemcpyAsync(w, a.sum, JG_AWT_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *total = (size_t)tot;
  const size_t k = std::min<size_t>(wcap, tot);
  if (k) HIPCHK(hipMemcpy(out, a.out, k * sizeof(jg_done_row), hipMemcpyDeviceToHost));
  if (k && !a.peek) t.cur ^= 1, t.n -= k;  // the survivors are in the other buffer
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
  for (size_t i = 0; i < n; i++) {
    const jg_await_row& r = rows[i];
    if (r.group >= e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_await_blocks: group out of range");
    if (r.flags || r.reserved) return fail(JG_EINVAL, "jg_engine_await_blocks: flags and reserved must be 0");
    if (!r.block_id) return fail(JG_EINVAL, "jg_engine_await_blocks: block id 0 is never applied");
  }
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
