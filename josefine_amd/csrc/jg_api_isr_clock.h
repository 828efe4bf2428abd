// jg_api_isr_clock.h - jg_engine_watch_replicas_timed: the replication feed under the time rule (jg_isr_clock.h).  A call
// that reads, in the shape of jg_api_isr.h: refused while kept node steps are outstanding, JG_NODE_ASYNC steps settled, the
// scratch carved from the engine's staging, a multi-device handle served shard by shard.  It shares the shadow with
// jg_engine_watch_replicas and keeps the clocks (stamps and their mask) next to it.  A call queues its passes back to back
// and synchronises once.  Part of josefine_gpu.hip's one translation unit.
#pragma once

namespace {

// one single-device engine's part of a timed replica watch: shard-local slots [g0, g0 + n); unless peeking the clocks of
// every slot of the range advance to c.now_ms; the first `cap` changed rows (groups + add) into host `out`, their shadow
// advanced unless peeking; *total the slots that differ.  cap 0 advances the clocks and delivers nothing
int isr_clock_shard(jg_engine* e, bool peek, const jg_isr_clock& c, uint32_t g0, uint32_t n, uint32_t add, jg_isr_row* out, size_t cap,
                    size_t* total) {
  *total = 0;
  if (!n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = node_settle(e);
    if (rc) return rc;
  }
  if (!e->isr_shadow) {  // (zero-filled on the engine's stream: no slot was last reported leading)
    const int rc = dev_alloc(e, &e->isr_shadow, e->cfg.n_groups);
    if (rc) return rc;
  }
  if (!e->isr_stamp) {  // (zero-filled: no member was behind at the last sample)
    if (const int rc = dev_alloc(e, &e->isr_stamp, (size_t)e->cfg.n_replicas * e->cfg.n_groups)) return rc;
  }
  if (!e->isr_behind) {
    if (const int rc = dev_alloc(e, &e->isr_behind, e->cfg.n_groups)) return rc;
  }
  const uint32_t tiles = (n + JG_ISR_TILE - 1) / JG_ISR_TILE;
  const size_t wcap = std::min<size_t>(cap, n);
  Carve cv;
  const size_t o_total = cv.sect(8), o_job = cv.sect(sizeof(JgScanJob)), o_cnt = cv.sect((size_t)tiles * 4), o_bsum = cv.sect((size_t)tiles * 8),
               o_out = cv.sect(wcap * sizeof(jg_isr_row));
  char* B = nullptr;
  if (const int rc = cv.on_staging(e, B)) return rc;
  JgIsrClockArgs a{};
  a.g0 = g0, a.n = n, a.add = add, a.peek = peek ? 1u : 0u;
  a.now1 = c.now_ms + 1, a.max_behind_ms = c.max_behind_ms, a.caught_lag = c.caught_lag, a.join_lag = c.join_lag;
  a.shadow = e->isr_shadow, a.stamp = e->isr_stamp, a.mask = e->isr_behind;
  a.cnt = (uint32_t*)(B + o_cnt);
  a.bsum = (uint64_t*)(B + o_bsum);
  a.out = (jg_isr_row*)(B + o_out);
  a.cap = wcap;
  const JgScanJob job{a.bsum, tiles, 0};
  HIPCHK(hipMemcpyAsync(B + o_job, &job, sizeof job, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_isrc_count, dim3(tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
  hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(JG_BLOCK), 0, e->stream, (const JgScanJob*)(B + o_job), (uint64_t*)(B + o_total));
  e->n_launch += 2;
  if (wcap) {  // (queued unseen: a quiet engine's workgroups return after their two loads)
    hipLaunchKernelGGL(k_isrc_write, dim3(tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
    e->n_launch++;
  }
  HIPCHK(hipGetLastError());
  uint64_t tot = 0;
  HIPCHK(hipMemcpyAsync(&tot, B + o_total, 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  *total = (size_t)tot;
  const size_t k = std::min<size_t>(wcap, tot);
  if (k) HIPCHK(hipMemcpy(out, a.out, k * sizeof(jg_isr_row), hipMemcpyDeviceToHost));
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_engine_watch_replicas_timed(jg_engine* e, uint32_t flags, const jg_isr_clock* c, uint32_t g0, uint32_t n, jg_isr_row* out, size_t cap,
                                   size_t* total) {
  if (!e || !c || !total || (cap && !out)) return fail(JG_EINVAL, "null argument");
  if (flags & ~(uint32_t)JG_WATCH_PEEK) return fail(JG_EINVAL, "jg_engine_watch_replicas_timed: unknown flag");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_watch_replicas_timed: slot range out of bounds");
  if (c->now_ms == UINT64_MAX) return fail(JG_EINVAL, "jg_engine_watch_replicas_timed: now_ms is UINT64_MAX");
  if (c->join_lag > c->caught_lag) return fail(JG_EINVAL, "jg_engine_watch_replicas_timed: join_lag above caught_lag");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  const bool peek = (flags & JG_WATCH_PEEK) != 0;
  const jg_isr_clock clk = *c;
  if (!e->router) return isr_clock_shard(e, peek, clk, g0, n, 0, out, cap, total);  // (straight into the caller's array)
  // a sharded handle: every shard is sized first by a pass that delivers nothing - and, unless peeking, advances ITS CLOCKS:
  // time passes on every shard, those behind the point where cap runs out too - then each shard delivers what is left of
  // cap behind the shards before it (its clocks advanced again at the same now_ms: nothing is stored)
  const size_t D = shard_count(e);
  std::vector<size_t> tot(D, 0), at(D + 1, 0);
  int rc = each_shard(e, [&](size_t d) -> int {
    const ShardPart sp = shard_part(e, d, g0, n);
    return isr_clock_shard(shard_at(e, d), peek, clk, sp.g0, sp.n, 0, nullptr, 0, &tot[d]);
  });
  if (rc) return rc;
  for (size_t d = 0; d < D; d++) at[d + 1] = at[d] + tot[d];
  *total = at[D];
  if (!cap || !at[D]) return JG_OK;
  return each_shard(e, [&](size_t d) -> int {
    if (!tot[d] || at[d] >= cap) return JG_OK;
    const ShardPart sp = shard_part(e, d, g0, n);
    size_t again = 0;
    return isr_clock_shard(shard_at(e, d), peek, clk, sp.g0, sp.n, e->router->lo[d], out + at[d], cap - at[d], &again);
  });
}

}  // extern "C"
