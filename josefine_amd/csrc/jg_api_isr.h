// jg_api_isr.h - jg_engine_watch_replicas / jg_engine_replication_census: the replication feed and its census (jg_isr.h).
// Calls that read, under the rules of jg_api_manage.h and in the shape of jg_api_watch.h: refused while kept node steps are
// outstanding, JG_NODE_ASYNC steps settled, the scratch carved from the engine's staging, a multi-device handle served
// shard by shard.  A call queues its passes back to back and synchronises once.  Part of josefine_gpu.hip's one
// translation unit.
#pragma once

namespace {

// one single-device engine's part of a replica watch: shard-local slots [g0, g0 + n), the first `cap` changed rows
// (groups + add) into host `out`, their shadow advanced unless peeking; *total the slots that differ
int isr_shard(jg_engine* e, bool peek, const jg_isr_policy& p, uint32_t g0, uint32_t n, uint32_t add, jg_isr_row* out, size_t cap,
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
  const uint32_t tiles = (n + JG_ISR_TILE - 1) / JG_ISR_TILE;
  const size_t wcap = std::min<size_t>(cap, n);
  Carve c;
  const size_t o_total = c.sect(8), o_job = c.sect(sizeof(JgScanJob)), o_cnt = c.sect((size_t)tiles * 4), o_bsum = c.sect((size_t)tiles * 8),
               o_out = c.sect(wcap * sizeof(jg_isr_row));
  char* B = nullptr;
  if (const int rc = c.on_staging(e, B)) return rc;
  JgIsrArgs a{};
  a.g0 = g0, a.n = n, a.add = add, a.peek = peek ? 1u : 0u;
  a.leave_lag = p.leave_lag, a.join_lag = p.join_lag;
  a.shadow = e->isr_shadow;
  a.cnt = (uint32_t*)(B + o_cnt);
  a.bsum = (uint64_t*)(B + o_bsum);
  a.out = (jg_isr_row*)(B + o_out);
  a.cap = wcap;
  const JgScanJob job{a.bsum, tiles, 0};
  HIPCHK(hipMemcpyAsync(B + o_job, &job, sizeof job, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_isr_count, dim3(tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
  hipLaunchKernelGGL(k_scan_block_sums, dim3(1), dim3(JG_BLOCK), 0, e->stream, (const JgScanJob*)(B + o_job), (uint64_t*)(B + o_total));
  e->n_launch += 2;
  if (wcap) {  // (queued unseen: a quiet engine's workgroups return after their two loads)
    hipLaunchKernelGGL(k_isr_write, dim3(tiles), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
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

// one single-device engine's part of a replication census: shard-local slots [g0, g0 + n) into w[JG_RC_WORDS]
int repl_census_shard(jg_engine* e, uint64_t lag_limit, uint32_t g0, uint32_t n, uint64_t* w) {
  std::memset(w, 0, JG_RC_WORDS * 8);
  if (!n) return JG_OK;
  HIPCHK(hipSetDevice(e->device));
  {
    const int rc = node_settle(e);
    if (rc) return rc;
  }
  JgReplCensusArgs a{};
  a.g0 = g0, a.n = n, a.lag_limit = lag_limit;
  a.tiles = (n + JG_REPL_CENSUS_TILE - 1) / JG_REPL_CENSUS_TILE;
  a.parts = std::min<uint32_t>(a.tiles, JG_REPL_CENSUS_PARTS);
  Carve c;
  const size_t o_out = c.sect(JG_RC_WORDS * 8), o_part = c.sect((size_t)a.parts * JG_RC_WORDS * 8);
  char* B = nullptr;
  if (const int rc = c.on_staging(e, B)) return rc;
  a.part = (uint64_t*)(B + o_part);
  a.out = (uint64_t*)(B + o_out);
  hipLaunchKernelGGL(k_repl_census, dim3(a.parts), dim3(JG_BLOCK), 0, e->stream, e->dev, a);
  hipLaunchKernelGGL(k_repl_census_sum, dim3(1), dim3(JG_BLOCK), 0, e->stream, a);
  e->n_launch += 2;
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(w, a.out, JG_RC_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return JG_OK;
}

}  // namespace

extern "C" {

int jg_engine_watch_replicas(jg_engine* e, uint32_t flags, const jg_isr_policy* p, uint32_t g0, uint32_t n, jg_isr_row* out, size_t cap,
                             size_t* total) {
  if (!e || !p || !total || (cap && !out)) return fail(JG_EINVAL, "null argument");
  if (flags & ~(uint32_t)JG_WATCH_PEEK) return fail(JG_EINVAL, "jg_engine_watch_replicas: unknown flag");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_watch_replicas: slot range out of bounds");
  if (p->join_lag > p->leave_lag) return fail(JG_EINVAL, "jg_engine_watch_replicas: join_lag above leave_lag");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  const bool peek = (flags & JG_WATCH_PEEK) != 0;
  const jg_isr_policy pol = *p;
  if (!e->router) return isr_shard(e, peek, pol, g0, n, 0, out, cap, total);  // (straight into the caller's array)
  // a sharded handle: every shard is sized first (a peek that delivers nothing), then each shard delivers - and advances -
  // what is left of cap behind the shards before it; a shard behind the point where cap ran out is not called again
  const size_t D = shard_count(e);
  std::vector<size_t> tot(D, 0), at(D + 1, 0);
  int rc = each_shard(e, [&](size_t d) -> int {
    const ShardPart sp = shard_part(e, d, g0, n);
    return isr_shard(shard_at(e, d), true, pol, sp.g0, sp.n, 0, nullptr, 0, &tot[d]);
  });
  if (rc) return rc;
  for (size_t d = 0; d < D; d++) at[d + 1] = at[d] + tot[d];
  *total = at[D];
  if (!cap || !at[D]) return JG_OK;
  return each_shard(e, [&](size_t d) -> int {
    if (!tot[d] || at[d] >= cap) return JG_OK;
    const ShardPart sp = shard_part(e, d, g0, n);
    size_t again = 0;
    return isr_shard(shard_at(e, d), peek, pol, sp.g0, sp.n, e->router->lo[d], out + at[d], cap - at[d], &again);
  });
}

int jg_engine_replication_census(jg_engine* e, uint64_t lag_limit, uint32_t g0, uint32_t n, jg_repl_census* out) {
  if (!e || !out) return fail(JG_EINVAL, "null argument");
  if ((uint64_t)g0 + n > e->cfg.n_groups) return fail(JG_EINVAL, "jg_engine_replication_census: slot range out of bounds");
  if (const int rc = refuse_first(e, kept_refuse)) return rc;
  const size_t D = shard_count(e);
  std::vector<uint64_t> w(D * JG_RC_WORDS, 0);
  const int rc = each_shard(e, [&](size_t d) -> int {
    const ShardPart sp = shard_part(e, d, g0, n);
    return repl_census_shard(shard_at(e, d), lag_limit, sp.g0, sp.n, w.data() + d * JG_RC_WORDS);
  });
  if (rc) return rc;
  uint64_t* o = (uint64_t*)out;  // (jg_repl_census is the census words in order: jg_isr.h)
  for (uint32_t x = 0; x < JG_RC_WORDS; x++) {
    uint64_t t = 0;
    for (size_t d = 0; d < D; d++) {
      const uint64_t v = w[d * JG_RC_WORDS + x];
      t = jg_rc_is_max(x) ? std::max(t, v) : t + v;
    }
    o[x] = t;
  }
  return JG_OK;
}

}  // extern "C"
